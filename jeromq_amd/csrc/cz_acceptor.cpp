// cz_acceptor.cpp -- the server half of the CURVE handshake for many connections at once (section 11
// of the header): N HELLO commands -> N WELCOME commands, N INITIATE commands -> N READY commands,
// each stage a fixed chain of device work whatever N is, ending in sessions cz_engine takes.
//
// Mirrors CurveServerMechanism.processHello :254-299, produceWelcome :301-358, processInitiate
// :360-471, produceReady :473-507 and produceError :509-517 item by item (no ZAP handler configured);
// the per-connection form of the same state machine is cz_curve_hs.cpp, whose metadata parser and
// Socket-Type table this file shares (cz_hs_parse.h).  The handle, the chain every stage runs and the
// entry points the client side has too are in cz_hs_batch.h.
//
// The stages' kernels, between the H2D copy and the D2H copy of that chain:
//   stage 1: k_x25519_jobs (3 lanes per connection: S' = s'.9, k1 = beforenm(C', s), cnPrecom =
//            beforenm(C', s')) | k_acc_welcome
//   stage 2: k_acc_initiate | k_x25519_jobs (k3 = beforenm(C, s'), gated on 2a's status) | k_acc_ready
// k1 serves the HELLO open and the WELCOME box; cnPrecom is computed in stage 1 so that stage 2 has
// one ladder on its critical path, not two ("Batched server handshake").  No key agreement runs twice for
// a connection.  The host side parses command framing before the launch and the metadata after it.
//
// Secrets: s', the cookie key and cnPrecom live in the device state table, indexed by slot, until
// cz_acceptor_release / destroy wipes the record.  The staging that carried them (pinned host and
// device, both directions) is wiped before a stage returns.  The cookie plaintext never leaves the
// device's registers.
#include <cstring>
#include <string>
#include <vector>

#include "cz_accept.h"
#include "cz_hs_batch.h"

using namespace czi;

namespace {

enum : uint8_t { SLOT_EXPECT_INITIATE = SLOT_WAITING };

const uint64_t NEXT_NONCE = 2;  // READY took cn_nonce 1

struct Slot {
    uint8_t state = SLOT_FREE;
    bool have_key = false;
    uint8_t client_key[32] = {};  // C, from an INITIATE whose boxes opened
    uint8_t precom[32] = {};      // cnPrecom, once CONNECTED
    uint64_t peer_nonce = 1;
    Props peer;

    void wipe()
    {
        secure_wipe(precom, 32);
        secure_wipe(client_key, 32);
        have_key = false;
        peer_nonce = 1;
        peer.clear();
        state = SLOT_FREE;
    }
};

}  // namespace

// konst: [0,32) the long-term secret s, [32, 32 + CZA_META_MAX) metadata; state: max_pending x CZA_STATE
struct cz_acceptor : HsBatch<Slot> {
    std::vector<uint8_t> meta;  // the metadata READY carries

    cz_acceptor() : HsBatch<Slot>("cz_acceptor", CZA_STATE) {}
};

extern "C" {

int cz_acceptor_create(cz_acceptor **out, const uint8_t secret_key[32], int socket_type, const uint8_t *identity,
                       uint32_t identity_len, uint32_t max_pending, int device)
{
    if (!out)
        return fail(CZ_EINVAL, "cz_acceptor_create: null pointer");
    *out = nullptr;
    if (!secret_key || (identity_len && !identity))
        return fail(CZ_EINVAL, "cz_acceptor_create: missing key");
    if (socket_type < 0 || socket_type >= sock_types())
        return fail(CZ_EINVAL, "cz_acceptor_create: unknown socket type %d", socket_type);
    if (max_pending == 0 || max_pending > (1u << 24))
        return fail(CZ_EINVAL, "cz_acceptor_create: max_pending %u outside 1 .. 2^24", max_pending);
    std::vector<uint8_t> meta = zmtp_metadata(socket_type, identity, identity_len);
    if (meta.size() > CZA_META_MAX)
        return fail(CZ_EMSGSIZE, "cz_acceptor_create: READY metadata of %zu bytes exceeds 256", meta.size());
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(CZ_EHIP, "no HIP device available (the CURVE path runs only on the GPU)");
    cz_acceptor *a = new cz_acceptor();
    a->meta = std::move(meta);
    uint8_t k[32 + CZA_META_MAX] = {};
    memcpy(k, secret_key, 32);
    memcpy(k + 32, a->meta.data(), a->meta.size());
    return hs_create(out, a, "cz_acceptor_create", k, sizeof k, socket_type, max_pending, device);
}

void cz_acceptor_destroy(cz_acceptor *a) { delete a; }

int cz_acceptor_hello(cz_acceptor *a, uint32_t count, const uint8_t *cmds, uint64_t cmds_bytes, const uint64_t *off,
                      const uint32_t *size, uint8_t *reply, uint64_t reply_stride, cz_accept_result *res,
                      const uint8_t *test_secrets, const uint8_t *test_entropy)
{
    if (!a)
        return fail(CZ_EINVAL, "cz_acceptor_hello: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!cmds || !off || !size || !reply || !res)
        return fail(CZ_EINVAL, "cz_acceptor_hello: null pointer");
    if (reply_stride < 168)
        return fail(CZ_EINVAL, "cz_acceptor_hello: reply_stride %llu below 168", (unsigned long long)reply_stride);
    if (!commands_inside(count, cmds_bytes, off, size))
        return fail(CZ_EINVAL, "cz_acceptor_hello: a command lies outside the %llu command bytes",
                    (unsigned long long)cmds_bytes);
    // 1. framing checks (processHello's, before its box) and a slot for every well-formed HELLO
    a->item.clear();
    for (uint32_t i = 0; i < count; i++) {
        res[i] = cz_accept_result{CZ_OK, 0, -1, 0};
        const uint8_t *m = cmds + off[i];
        if (!starts_with(m, size[i], "HELLO")) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_UNEXPECTED_COMMAND;
        } else if (size[i] != 200 || m[6] != 1 || m[7] != 0) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_MALFORMED_COMMAND_HELLO;
        } else if (a->free_slots.empty()) {
            res[i].rc = CZ_EAGAIN;
        } else {
            res[i].slot = a->free_slots.back();
            a->free_slots.pop_back();
            a->item.push_back(i);
        }
    }
    const uint32_t nj = (uint32_t)a->item.size();
    if (nj == 0)
        return CZ_OK;
    // 2. the records, and three key agreements per record into x (the output is the WELCOME: no secret)
    Stage<Slot> st(*a, "cz_acceptor_hello", nj, LaneShape{3, CZA_IN1, CZA_X1, CZA_OUT1}, false, res);
    int rc = st.reserve();
    if (rc != CZ_OK)
        return rc;
    const StageBuffers sb = st.buffers();
    const uint8_t *d_key = (const uint8_t *)a->konst.ptr;
    cza_job *jobs = sb.jobs;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = sb.recs + (uint64_t)CZA_IN1 * j;
        memcpy(r + CZA_IN1_CP, m + 80, 32);
        memcpy(r + CZA_IN1_NONCE, m + 112, 8);
        memcpy(r + CZA_IN1_BOX, m + 120, 80);
        static_assert(CZA_IN1_SECRET == CZA_IN1_ENTROPY + 64, "entropy and s' are drawn in one call");
        if (!test_entropy && !test_secrets) {
            rc = fill_random(r + CZA_IN1_ENTROPY, 96, a->name);
        } else {
            if (test_entropy)
                memcpy(r + CZA_IN1_ENTROPY, test_entropy + 64ull * i, 64);
            else
                rc = fill_random(r + CZA_IN1_ENTROPY, 64, a->name);
            if (test_secrets)
                memcpy(r + CZA_IN1_SECRET, test_secrets + 32ull * i, 32);
            else if (rc == CZ_OK)
                rc = fill_random(r + CZA_IN1_SECRET, 32, a->name);
        }
        const int32_t slot = res[i].slot;
        memcpy(r + CZA_IN1_SLOT, &slot, 4);
        const uint8_t *dr = sb.d_recs + (uint64_t)CZA_IN1 * j;
        uint8_t *dx = sb.d_x + (uint64_t)CZA_X1 * j;
        jobs[3 * j] = cza_job{dr + CZA_IN1_SECRET, nullptr, dx, nullptr, CZA_JOB_BASE, 0};                    // S'
        jobs[3 * j + 1] = cza_job{d_key, dr + CZA_IN1_CP, dx + 32, nullptr, CZA_JOB_BEFORENM, 0};             // k1
        jobs[3 * j + 2] = cza_job{dr + CZA_IN1_SECRET, dr + CZA_IN1_CP, dx + 64, nullptr, CZA_JOB_BEFORENM, 0};  // cnPrecom
    }
    if (rc != CZ_OK)
        return st.abandon(rc);
    rc = st.run([=](hipStream_t s) {
        const hipError_t e = czk_x25519_jobs(sb.d_jobs, 3 * nj, s);
        return e != hipSuccess ? e : czk_acc_welcome(sb.d_recs, sb.d_x, sb.d_out, a->state.ptr, nj, s);
    });
    if (rc != CZ_OK)
        return rc;
    for (uint32_t j = 0; j < nj; j++)  // the staged secrets: cookie key and s' (the rest came off the wire)
        secure_wipe(sb.recs + (uint64_t)CZA_IN1 * j + CZA_IN1_ENTROPY, 96);
    // 3. results: WELCOME and a pending slot, or ERROR (processHello's failed open, produceError)
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *o = sb.out + (uint64_t)CZA_OUT1 * j;
        uint8_t *rp = reply + reply_stride * i;
        const uint32_t status = st.status(j, o + CZA_OUT1_STATUS, res[i]);
        if (status == CZA_ST_OK) {
            memcpy(rp, o + CZA_OUT1_CMD, 168);
            res[i].reply_len = 168;
            a->slots[(size_t)res[i].slot].state = SLOT_EXPECT_INITIATE;
            continue;
        }
        if (status == CZA_ST_CRYPTO) {
            memcpy(rp, "\x05" "ERROR\x00", 7);
            res[i].reply_len = 7;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
        }
        a->free_slot(res[i].slot);
        res[i].slot = -1;
    }
    return st.rc;
}

int cz_acceptor_initiate(cz_acceptor *a, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                         const uint64_t *off, const uint32_t *size, uint8_t *reply, uint64_t reply_stride,
                         cz_accept_result *res)
{
    if (!a)
        return fail(CZ_EINVAL, "cz_acceptor_initiate: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!slot || !cmds || !off || !size || !reply || !res)
        return fail(CZ_EINVAL, "cz_acceptor_initiate: null pointer");
    if (reply_stride < 288)
        return fail(CZ_EINVAL, "cz_acceptor_initiate: reply_stride %llu below 288", (unsigned long long)reply_stride);
    if (!commands_inside(count, cmds_bytes, off, size))
        return fail(CZ_EINVAL, "cz_acceptor_initiate: a command lies outside the %llu command bytes",
                    (unsigned long long)cmds_bytes);
    // 1. slot state and processInitiate's framing checks; every slot named here leaves EXPECT_INITIATE
    a->item.clear();
    for (uint32_t i = 0; i < count; i++) {
        res[i] = cz_accept_result{CZ_OK, 0, slot[i], 0};
        Slot *s = a->slot(slot[i]);
        if (!s || s->state != SLOT_EXPECT_INITIATE) {
            res[i].rc = CZ_EINVAL;
            res[i].slot = -1;
            continue;
        }
        s->state = SLOT_FAILED;
        const uint8_t *m = cmds + off[i];
        if (!starts_with(m, size[i], "INITIATE")) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_UNEXPECTED_COMMAND;
        } else if (size[i] < 257 || (uint64_t)size[i] - 113 + 16 > 16 + 144 + 256) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_MALFORMED_COMMAND_INITIATE;
        } else {
            a->item.push_back(i);
        }
    }
    const uint32_t nj = (uint32_t)a->item.size();
    if (nj == 0)
        return CZ_OK;
    // 2. the records, and one key agreement per record into x (the output carries cnPrecom)
    Stage<Slot> st(*a, "cz_acceptor_initiate", nj, LaneShape{1, CZA_IN2, 32, CZA_OUT2}, true, nullptr);
    int rc = st.reserve();
    if (rc != CZ_OK)
        return rc;
    const StageBuffers sb = st.buffers();
    const uint8_t *d_state = (const uint8_t *)a->state.ptr;
    cza_job *jobs = sb.jobs;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = sb.recs + (uint64_t)CZA_IN2 * j;
        const uint32_t plain_len = size[i] - 113 - 16;  // 128 .. CZA_INIT_MAX
        memcpy(r + CZA_IN2_SLOT, &slot[i], 4);
        memcpy(r + CZA_IN2_LEN, &plain_len, 4);
        memcpy(r + CZA_IN2_NONCE, m + 105, 8);
        memcpy(r + CZA_IN2_COOKIE_NONCE, m + 9, 16);
        memcpy(r + CZA_IN2_COOKIE, m + 25, 80);
        memcpy(r + CZA_IN2_BOX, m + 113, size[i] - 113);
        memset(r + CZA_IN2_BOX + 16 + plain_len, 0, (0u - plain_len) & 15u);  // the last chunk's pad
        uint8_t *dout = sb.d_out + (uint64_t)CZA_OUT2 * j;
        // k3 = beforenm(C, s'): the vouch's key, once 2a has opened the box that holds C
        jobs[j] = cza_job{d_state + (uint64_t)CZA_STATE * (uint32_t)slot[i] + CZA_STATE_SECRET, dout + CZA_OUT2_PLAIN,
                          sb.d_x + 32ull * j, (const uint32_t *)(dout + CZA_OUT2_STATUS), CZA_JOB_BEFORENM, 0};
    }
    rc = st.run([=](hipStream_t s) {
        hipError_t e;
        if ((e = czk_acc_initiate(sb.d_recs, sb.d_out, d_state, nj, s)) != hipSuccess ||
            (e = czk_x25519_jobs(sb.d_jobs, nj, s)) != hipSuccess)
            return e;
        return czk_acc_ready(sb.d_out, sb.d_x, sb.d_recs, d_state, (const uint8_t *)a->konst.ptr + 32,
                             (uint32_t)a->meta.size(), nj, s);
    });
    if (rc != CZ_OK)
        return rc;
    // 3. results: the metadata (Metadata.read + the Socket-Type check) on the host, then READY
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        uint8_t *o = sb.out + (uint64_t)CZA_OUT2 * j;
        Slot &s = a->slots[(size_t)slot[i]];
        const uint32_t status = st.status(j, o + CZA_OUT2_STATUS, res[i], {CZA_ST_OK, CZA_ST_CRYPTO, CZA_ST_KEY_EXCHANGE});
        if (status == CZA_ST_CRYPTO || status == CZA_ST_KEY_EXCHANGE) {
            res[i].rc = CZ_EPROTO;
            res[i].event = status == CZA_ST_KEY_EXCHANGE ? CZ_ZMTP_KEY_EXCHANGE : CZ_ZMTP_CRYPTOGRAPHIC;
        }
        if (status != CZA_ST_OK)
            continue;
        const uint8_t *m = cmds + off[i];
        const uint32_t plain_len = size[i] - 113 - 16;
        memcpy(s.client_key, o + CZA_OUT2_PLAIN, 32);
        s.have_key = true;
        s.peer.clear();
        const int mrc = parse_metadata(o + CZA_OUT2_PLAIN + 128, plain_len - 128, a->socket_type, &s.peer);
        if (mrc != CZ_OK) {
            res[i].rc = mrc;
            continue;
        }
        memcpy(s.precom, o + CZA_OUT2_PRECOM, 32);
        secure_wipe(o + CZA_OUT2_PRECOM, 32);
        s.peer_nonce = get_be64(m + 105);
        s.state = SLOT_CONNECTED;
        uint8_t *rp = reply + reply_stride * i;
        memcpy(rp, "\x05READY", 6);
        put_be64(rp + 6, 1);  // cn_nonce = 1; the session continues at NEXT_NONCE
        memcpy(rp + 14, o + CZA_OUT2_READY, 16 + a->meta.size());
        res[i].reply_len = (uint32_t)(14 + 16 + a->meta.size());
    }
    // (stage 2 stages no secret towards the device; what came back held cnPrecom, wiped above, and
    // for lanes whose metadata failed, wiped here)
    for (uint32_t j = 0; j < nj; j++)
        if (a->slots[(size_t)slot[a->item[j]]].state != SLOT_CONNECTED)
            secure_wipe(sb.out + (uint64_t)CZA_OUT2 * j + CZA_OUT2_PRECOM, 32);
    return st.rc;
}

int cz_acceptor_session(const cz_acceptor *a, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                        uint64_t *cn_peer_nonce)
{
    return hs_session(a, "cz_acceptor_session", slot, precom, cn_nonce, cn_peer_nonce, NEXT_NONCE);
}

int cz_acceptor_client_key(const cz_acceptor *a, int32_t slot, uint8_t key[32])
{
    const Slot *s = a && key ? a->slot(slot) : nullptr;
    if (!s || !s->have_key)
        return fail(CZ_EINVAL, "cz_acceptor_client_key: no INITIATE opened on slot %d", slot);
    memcpy(key, s->client_key, 32);
    return CZ_OK;
}

int cz_acceptor_peer_property(const cz_acceptor *a, int32_t slot, const char *name, const uint8_t **value, uint32_t *len)
{
    return hs_peer_property(a, "cz_acceptor_peer_property", slot, name, value, len);
}

int cz_engine_add_accepted(cz_engine *e, const cz_acceptor *a, int32_t slot)
{
    return hs_engine_add(e, a, "cz_acceptor_session", slot, NEXT_NONCE, 1);
}

// (the device record holds s', the cookie key and cnPrecom)
int cz_acceptor_release(cz_acceptor *a, int32_t slot) { return hs_release(a, "cz_acceptor_release", slot); }

int cz_engine_add_accepted_batch(cz_engine *e, const cz_acceptor *a, uint32_t count, const int32_t *slots, int32_t *ids)
{
    return hs_engine_add_batch(e, a, "cz_engine_add_accepted_batch", count, slots, ids, CZA_STATE_PRECOM, NEXT_NONCE, 1);
}

int cz_acceptor_release_batch(cz_acceptor *a, uint32_t count, const int32_t *slots)
{
    return hs_release_batch(a, "cz_acceptor_release_batch", count, slots);
}

uint32_t cz_acceptor_pending(const cz_acceptor *a) { return hs_pending(a); }

}  // extern "C"
