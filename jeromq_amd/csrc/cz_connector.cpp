// cz_connector.cpp -- the client half of the CURVE handshake for many connections at once (section 12
// of the header): N server keys -> N HELLO commands, N WELCOME commands -> N INITIATE commands, N READY
// commands -> N sessions cz_engine takes, each stage a fixed chain of device work whatever N is.
//
// Mirrors CurveClientMechanism.produceHello :246-279, processWelcome :281-316, produceInitiate
// :318-385, processReady :387-419 and processError :421-429 item by item; the per-connection form of
// the same state machine is cz_curve_hs.cpp, and the command dispatch, the framing checks, the ERROR
// parse and the metadata parser are the functions it calls (cz_hs_parse.h).  The handle, the chain
// every stage runs and the entry points the server side has too are in cz_hs_batch.h.
//
// The stages' kernels, between the H2D copy and the D2H copy of that chain:
//   hello:   k_x25519_jobs (2 lanes per connection: C' = c'.9, kH = beforenm(S, c')) | k_con_hello
//   welcome: k_con_welcome | k_x25519_jobs (2 lanes per connection, gated on the open's status:
//            cnPrecom = beforenm(S', c'), kV = beforenm(S', c)) | k_con_initiate
//   ready:   k_con_ready (no key agreement: no jobs and no x)
// kH seals the HELLO box and opens the WELCOME box; cnPrecom seals the INITIATE box, opens the READY
// box and is the session key.  No key agreement runs twice for a connection (cz_hs runs six ladders).
//
// Secrets: c', kH, cnPrecom and kV live in the device state table, indexed by slot.  k_con_initiate
// wipes c', kH and kV once the INITIATE is made; cz_connector_release / destroy wipes the record.  The
// staging that carried c' (pinned host and device) or cnPrecom is wiped before a stage returns.
#include <cstring>
#include <string>
#include <vector>

#include "cz_connect.h"
#include "cz_hs_batch.h"

using namespace czi;

namespace {

enum : uint8_t { SLOT_EXPECT_WELCOME = SLOT_WAITING, SLOT_EXPECT_READY };

const uint64_t NEXT_NONCE = 3;  // HELLO took cn_nonce 1, INITIATE 2

struct Slot {
    uint8_t state = SLOT_FREE;
    uint8_t server_key[32] = {};  // S, as given to cz_connector_hello
    uint8_t cn_public[32] = {};   // C', from the HELLO the device made
    uint8_t precom[32] = {};      // cnPrecom, once CONNECTED
    uint64_t peer_nonce = 1;
    int auth_status = 0;          // status code of an ERROR command (handleErrorReason)
    Props peer;

    void wipe()
    {
        secure_wipe(precom, 32);
        memset(server_key, 0, 32);
        memset(cn_public, 0, 32);
        peer_nonce = 1;
        auth_status = 0;
        peer.clear();
        state = SLOT_FREE;
    }
};

}  // namespace

// konst: CZC_KONST bytes, the long-term secret c, C, the metadata; state: max_pending x CZC_STATE
struct cz_connector : HsBatch<Slot> {
    uint32_t meta_len = 0;  // the metadata INITIATE carries

    cz_connector() : HsBatch<Slot>("cz_connector", CZC_STATE) {}

    // What a slot waiting for `want` makes of command m: true if it goes to the device.  Otherwise res
    // holds what a cz_hs client in that state returns for it (processHandshakeCommand's dispatch, the
    // size checks, processError).  Every slot named in a stage leaves the state it was in.
    bool frame(Slot &s, ClientCommand want, const uint8_t *m, uint32_t size, cz_accept_result &res)
    {
        s.state = SLOT_FAILED;
        const ClientCommand got = client_command(m, size);
        if (got == CLIENT_CMD_ERROR) {
            int ev = 0;
            res.rc = parse_error_command(m, size, &s.auth_status, &ev);
            res.event = ev;
            return false;
        }
        int ev = CZ_ZMTP_UNEXPECTED_COMMAND;
        if (got == want)
            ev = want == CLIENT_CMD_WELCOME ? welcome_framing(size) : ready_framing(size);
        if (ev) {
            res.rc = CZ_EPROTO;
            res.event = ev;
            return false;
        }
        return true;
    }
};

extern "C" {

int cz_connector_create(cz_connector **out, const uint8_t public_key[32], const uint8_t secret_key[32], int socket_type,
                        const uint8_t *identity, uint32_t identity_len, uint32_t max_pending, int device)
{
    if (!out)
        return fail(CZ_EINVAL, "cz_connector_create: null pointer");
    *out = nullptr;
    if (!public_key || !secret_key || (identity_len && !identity))
        return fail(CZ_EINVAL, "cz_connector_create: missing key");
    if (socket_type < 0 || socket_type >= sock_types())
        return fail(CZ_EINVAL, "cz_connector_create: unknown socket type %d", socket_type);
    if (max_pending == 0 || max_pending > (1u << 24))
        return fail(CZ_EINVAL, "cz_connector_create: max_pending %u outside 1 .. 2^24", max_pending);
    const std::vector<uint8_t> meta = zmtp_metadata(socket_type, identity, identity_len);
    if (meta.size() > CZC_META_MAX)  // "Assume here that metadata is limited to 256 bytes"
        return fail(CZ_EMSGSIZE, "cz_connector_create: INITIATE metadata of %zu bytes exceeds 256", meta.size());
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(CZ_EHIP, "no HIP device available (the CURVE path runs only on the GPU)");
    cz_connector *c = new cz_connector();
    c->meta_len = (uint32_t)meta.size();
    uint8_t k[CZC_KONST] = {};
    memcpy(k + CZC_KONST_SECRET, secret_key, 32);
    memcpy(k + CZC_KONST_PUBLIC, public_key, 32);
    memcpy(k + CZC_KONST_META, meta.data(), meta.size());
    return hs_create(out, c, "cz_connector_create", k, sizeof k, socket_type, max_pending, device);
}

void cz_connector_destroy(cz_connector *c) { delete c; }

int cz_connector_hello(cz_connector *c, uint32_t count, const uint8_t *server_keys, uint8_t *reply, uint64_t reply_stride,
                       cz_accept_result *res, const uint8_t *test_secrets)
{
    if (!c)
        return fail(CZ_EINVAL, "cz_connector_hello: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!server_keys || !reply || !res)
        return fail(CZ_EINVAL, "cz_connector_hello: null pointer");
    if (reply_stride < 200)
        return fail(CZ_EINVAL, "cz_connector_hello: reply_stride %llu below 200", (unsigned long long)reply_stride);
    // 1. a slot for every connection the table has room for
    c->item.clear();
    for (uint32_t i = 0; i < count; i++) {
        res[i] = cz_accept_result{CZ_OK, 0, -1, 0};
        if (c->free_slots.empty()) {
            res[i].rc = CZ_EAGAIN;
        } else {
            res[i].slot = c->free_slots.back();
            c->free_slots.pop_back();
            c->item.push_back(i);
        }
    }
    const uint32_t nj = (uint32_t)c->item.size();
    if (nj == 0)
        return CZ_OK;
    // 2. the records, and two key agreements per record into x (the output is the HELLO: no secret)
    Stage<Slot> st(*c, "cz_connector_hello", nj, LaneShape{2, CZC_IN1, CZC_X1, CZC_OUT1}, false, res);
    int rc = st.reserve();
    if (rc != CZ_OK)
        return rc;
    const StageBuffers sb = st.buffers();
    cza_job *jobs = sb.jobs;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = c->item[j];
        uint8_t *r = sb.recs + (uint64_t)CZC_IN1 * j;
        memcpy(r + CZC_IN1_SERVER, server_keys + 32ull * i, 32);
        if (test_secrets)
            memcpy(r + CZC_IN1_SECRET, test_secrets + 32ull * i, 32);
        else
            rc = fill_random(r + CZC_IN1_SECRET, 32, c->name);
        const int32_t slot = res[i].slot;
        memcpy(r + CZC_IN1_SLOT, &slot, 4);
        memset(r + CZC_IN1_SLOT + 4, 0, CZC_IN1 - CZC_IN1_SLOT - 4);
        const uint8_t *dr = sb.d_recs + (uint64_t)CZC_IN1 * j;
        uint8_t *dx = sb.d_x + (uint64_t)CZC_X1 * j;
        jobs[2 * j] = cza_job{dr + CZC_IN1_SECRET, nullptr, dx, nullptr, CZA_JOB_BASE, 0};                           // C'
        jobs[2 * j + 1] = cza_job{dr + CZC_IN1_SECRET, dr + CZC_IN1_SERVER, dx + 32, nullptr, CZA_JOB_BEFORENM, 0};  // kH
    }
    if (rc != CZ_OK)
        return st.abandon(rc);
    rc = st.run([=](hipStream_t s) {
        const hipError_t e = czk_x25519_jobs(sb.d_jobs, 2 * nj, s);
        return e != hipSuccess ? e : czk_con_hello(sb.d_recs, sb.d_x, sb.d_out, c->state.ptr, nj, s);
    });
    if (rc != CZ_OK)
        return rc;
    for (uint32_t j = 0; j < nj; j++)  // the staged secret: c' (the rest is public)
        secure_wipe(sb.recs + (uint64_t)CZC_IN1 * j + CZC_IN1_SECRET, 32);
    // 3. results: the HELLO and a slot that waits for its WELCOME
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = sb.out + (uint64_t)CZC_OUT1 * j;
        if (st.status(j, o + CZC_OUT1_STATUS, res[i], {CZA_ST_OK}) == CZA_ST_OK) {
            Slot &s = c->slots[(size_t)res[i].slot];
            memcpy(reply + reply_stride * i, o + CZC_OUT1_CMD, 200);
            res[i].reply_len = 200;
            memcpy(s.server_key, server_keys + 32ull * i, 32);
            memcpy(s.cn_public, o + CZC_OUT1_CMD + 80, 32);
            s.state = SLOT_EXPECT_WELCOME;
        } else {
            (void)c->wipe_record(res[i].slot);
            c->free_slot(res[i].slot);
            res[i].slot = -1;
        }
    }
    return st.rc;
}

int cz_connector_welcome(cz_connector *c, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                         const uint64_t *off, const uint32_t *size, uint8_t *reply, uint64_t reply_stride,
                         cz_accept_result *res, const uint8_t *test_entropy)
{
    if (!c)
        return fail(CZ_EINVAL, "cz_connector_welcome: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!slot || !cmds || !off || !size || !reply || !res)
        return fail(CZ_EINVAL, "cz_connector_welcome: null pointer");
    if (reply_stride < CZC_INITIATE_MAX)
        return fail(CZ_EINVAL, "cz_connector_welcome: reply_stride %llu below %d", (unsigned long long)reply_stride,
                    CZC_INITIATE_MAX);
    if (!commands_inside(count, cmds_bytes, off, size))
        return fail(CZ_EINVAL, "cz_connector_welcome: a command lies outside the %llu command bytes",
                    (unsigned long long)cmds_bytes);
    // 1. slot state, the command's name and processWelcome's size check; every slot named here leaves
    //    EXPECT_WELCOME (a slot named twice: the first item takes it, the second finds it gone)
    c->item.clear();
    for (uint32_t i = 0; i < count; i++) {
        res[i] = cz_accept_result{CZ_OK, 0, slot[i], 0};
        Slot *s = c->slot(slot[i]);
        if (!s || s->state != SLOT_EXPECT_WELCOME) {
            res[i].rc = CZ_EINVAL;
            res[i].slot = -1;
            continue;
        }
        if (c->frame(*s, CLIENT_CMD_WELCOME, cmds + off[i], size[i], res[i]))
            c->item.push_back(i);
    }
    const uint32_t nj = (uint32_t)c->item.size();
    if (nj == 0)
        return CZ_OK;
    // 2. the records, and two key agreements per record, from S' in the x scratch into the slot table
    Stage<Slot> st(*c, "cz_connector_welcome", nj, LaneShape{2, CZC_IN2, CZC_X2, CZC_OUT2}, true, nullptr);
    int rc = st.reserve();
    if (rc != CZ_OK)
        return rc;
    uint8_t *d_state = (uint8_t *)c->state.ptr;
    const uint8_t *d_konst = (const uint8_t *)c->konst.ptr;
    const StageBuffers sb = st.buffers();
    cza_job *jobs = sb.jobs;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *m = cmds + off[i];
        const Slot &s = c->slots[(size_t)slot[i]];
        uint8_t *r = sb.recs + (uint64_t)CZC_IN2 * j;
        memset(r, 0, CZC_IN2_NONCE);
        memcpy(r + CZC_IN2_SLOT, &slot[i], 4);
        memcpy(r + CZC_IN2_NONCE, m + 8, 16);
        memcpy(r + CZC_IN2_BOX, m + 24, 144);
        memcpy(r + CZC_IN2_SERVER, s.server_key, 32);
        memcpy(r + CZC_IN2_CP, s.cn_public, 32);
        if (test_entropy)
            memcpy(r + CZC_IN2_VNONCE, test_entropy + 16ull * i, 16);
        else
            rc = fill_random(r + CZC_IN2_VNONCE, 16, c->name);
        uint8_t *sr = d_state + (uint64_t)CZC_STATE * (uint32_t)slot[i];
        const uint8_t *sp = sb.d_x + (uint64_t)CZC_X2 * j + CZC_X2_SP;
        const uint32_t *gate = (const uint32_t *)(sb.d_out + (uint64_t)CZC_OUT2 * j + CZC_OUT2_STATUS);
        // once 2a has opened the box that holds S': the session key and the vouch's key, into the slot
        jobs[2 * j] = cza_job{sr + CZC_STATE_SECRET, sp, sr + CZC_STATE_PRECOM, gate, CZA_JOB_BEFORENM, 0};
        jobs[2 * j + 1] = cza_job{d_konst + CZC_KONST_SECRET, sp, sr + CZC_STATE_KV, gate, CZA_JOB_BEFORENM, 0};
    }
    if (rc != CZ_OK)
        return st.abandon(rc);
    rc = st.run([=](hipStream_t s) {
        hipError_t e;
        if ((e = czk_con_welcome(sb.d_recs, sb.d_out, sb.d_x, d_state, nj, s)) != hipSuccess ||
            (e = czk_x25519_jobs(sb.d_jobs, 2 * nj, s)) != hipSuccess)
            return e;
        return czk_con_initiate(sb.d_out, sb.d_x, sb.d_recs, d_state, d_konst, c->meta_len, nj, s);
    });
    if (rc != CZ_OK)
        return rc;
    // 3. results: the INITIATE and a slot that waits for its READY
    // (this stage stages no secret through the host: the keys went from the ladder into the slot table)
    const uint32_t init_len = 113 + 16 + 128 + c->meta_len;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = sb.out + (uint64_t)CZC_OUT2 * j;
        const uint32_t status = st.status(j, o + CZC_OUT2_STATUS, res[i]);
        if (status == CZA_ST_OK) {
            memcpy(reply + reply_stride * i, o + CZC_OUT2_CMD, init_len);
            res[i].reply_len = init_len;
            c->slots[(size_t)slot[i]].state = SLOT_EXPECT_READY;
        } else if (status == CZA_ST_CRYPTO) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
        }
    }
    return st.rc;
}

int cz_connector_ready(cz_connector *c, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                       const uint64_t *off, const uint32_t *size, cz_accept_result *res)
{
    if (!c)
        return fail(CZ_EINVAL, "cz_connector_ready: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!slot || !cmds || !off || !size || !res)
        return fail(CZ_EINVAL, "cz_connector_ready: null pointer");
    if (!commands_inside(count, cmds_bytes, off, size))
        return fail(CZ_EINVAL, "cz_connector_ready: a command lies outside the %llu command bytes",
                    (unsigned long long)cmds_bytes);
    // 1. slot state, the command's name and processReady's size checks; every slot named here leaves
    //    EXPECT_READY
    c->item.clear();
    for (uint32_t i = 0; i < count; i++) {
        res[i] = cz_accept_result{CZ_OK, 0, slot[i], 0};
        Slot *s = c->slot(slot[i]);
        if (!s || s->state != SLOT_EXPECT_READY) {
            res[i].rc = CZ_EINVAL;
            res[i].slot = -1;
            continue;
        }
        if (c->frame(*s, CLIENT_CMD_READY, cmds + off[i], size[i], res[i]))
            c->item.push_back(i);
    }
    const uint32_t nj = (uint32_t)c->item.size();
    if (nj == 0)
        return CZ_OK;
    // 2. the records (the output carries cnPrecom)
    Stage<Slot> st(*c, "cz_connector_ready", nj, LaneShape{0, CZC_IN3, 0, CZC_OUT3}, true, nullptr);
    int rc = st.reserve();
    if (rc != CZ_OK)
        return rc;
    const StageBuffers sb = st.buffers();
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = sb.recs + (uint64_t)CZC_IN3 * j;
        const uint32_t plain_len = size[i] - 14 - 16;  // 0 .. CZC_READY_MAX
        memcpy(r + CZC_IN3_SLOT, &slot[i], 4);
        memcpy(r + CZC_IN3_LEN, &plain_len, 4);
        memcpy(r + CZC_IN3_NONCE, m + 6, 8);
        memcpy(r + CZC_IN3_BOX, m + 14, size[i] - 14);
        memset(r + CZC_IN3_BOX + 16 + plain_len, 0, (0u - plain_len) & 15u);  // the last chunk's pad
    }
    rc = st.run([=](hipStream_t s) { return czk_con_ready(sb.d_recs, sb.d_out, c->state.ptr, nj, s); });
    if (rc != CZ_OK)
        return rc;
    // 3. results: the metadata (Metadata.read + the Socket-Type check) on the host, then the session
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = sb.out + (uint64_t)CZC_OUT3 * j;
        Slot &s = c->slots[(size_t)slot[i]];
        const uint32_t status = st.status(j, o + CZC_OUT3_STATUS, res[i]);
        if (status == CZA_ST_CRYPTO) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
        }
        if (status != CZA_ST_OK)
            continue;
        s.peer.clear();
        const int mrc = parse_metadata(o + CZC_OUT3_PLAIN, size[i] - 14 - 16, c->socket_type, &s.peer);
        if (mrc != CZ_OK) {
            res[i].rc = mrc;
            continue;
        }
        memcpy(s.precom, o + CZC_OUT3_PRECOM, 32);
        s.peer_nonce = get_be64(cmds + off[i] + 6);
        s.state = SLOT_CONNECTED;
    }
    secure_wipe(sb.out, st.out_bytes());  // it held cnPrecom
    return st.rc;
}

int cz_connector_session(const cz_connector *c, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                         uint64_t *cn_peer_nonce)
{
    return hs_session(c, "cz_connector_session", slot, precom, cn_nonce, cn_peer_nonce, NEXT_NONCE);
}

int cz_connector_peer_property(const cz_connector *c, int32_t slot, const char *name, const uint8_t **value,
                               uint32_t *len)
{
    return hs_peer_property(c, "cz_connector_peer_property", slot, name, value, len);
}

int cz_connector_error_status(const cz_connector *c, int32_t slot)
{
    const Slot *s = c ? c->slot(slot) : nullptr;
    return s && s->state != SLOT_FREE ? s->auth_status : 0;
}

int cz_connector_server_key(const cz_connector *c, int32_t slot, uint8_t key[32])
{
    const Slot *s = c && key ? c->slot(slot) : nullptr;
    if (!s || s->state == SLOT_FREE)
        return fail(CZ_EINVAL, "cz_connector_server_key: slot %d is not in use", slot);
    memcpy(key, s->server_key, 32);
    return CZ_OK;
}

int cz_engine_add_connected(cz_engine *e, const cz_connector *c, int32_t slot)
{
    return hs_engine_add(e, c, "cz_connector_session", slot, NEXT_NONCE, 0);
}

// (the device record holds c', kH, cnPrecom and kV)
int cz_connector_release(cz_connector *c, int32_t slot) { return hs_release(c, "cz_connector_release", slot); }

int cz_engine_add_connected_batch(cz_engine *e, const cz_connector *c, uint32_t count, const int32_t *slots, int32_t *ids)
{
    return hs_engine_add_batch(e, c, "cz_engine_add_connected_batch", count, slots, ids, CZC_STATE_PRECOM, NEXT_NONCE, 0);
}

int cz_connector_release_batch(cz_connector *c, uint32_t count, const int32_t *slots)
{
    return hs_release_batch(c, "cz_connector_release_batch", count, slots);
}

uint32_t cz_connector_pending(const cz_connector *c) { return hs_pending(c); }

}  // extern "C"
