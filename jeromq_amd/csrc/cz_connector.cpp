// cz_connector.cpp -- the client half of the CURVE handshake for many connections at once (section 12
// of the header): N server keys -> N HELLO commands, N WELCOME commands -> N INITIATE commands, N READY
// commands -> N sessions cz_engine takes, each stage a fixed chain of device work whatever N is.
//
// Mirrors CurveClientMechanism.produceHello :246-279, processWelcome :281-316, produceInitiate
// :318-385, processReady :387-419 and processError :421-429 item by item; the per-connection form of
// the same state machine is cz_curve_hs.cpp, and the command dispatch, the framing checks, the ERROR
// parse and the metadata parser are the functions it calls (cz_hs_parse.h).
//
// Launch chain (one stream, one synchronisation per stage):
//   hello:   H2D jobs + records | k_x25519_jobs (2 lanes per connection: C' = c'.9, kH = beforenm(S, c'))
//            | k_con_hello | D2H out | wipe | sync
//   welcome: memset out | H2D jobs + records | k_con_welcome | k_x25519_jobs (2 lanes per connection,
//            gated on the open's status: cnPrecom = beforenm(S', c'), kV = beforenm(S', c)) |
//            k_con_initiate | D2H out | wipe | sync
//   ready:   memset out | H2D records | k_con_ready | D2H out | wipe | sync
// kH seals the HELLO box and opens the WELCOME box; cnPrecom seals the INITIATE box, opens the READY
// box and is the session key.  No key agreement runs twice for a connection (cz_hs runs six ladders).
//
// Secrets: c', kH, cnPrecom and kV live in the device state table, indexed by slot.  k_con_initiate
// wipes c', kH and kV once the INITIATE is made; cz_connector_release / destroy wipes the record.  The
// staging that carried c' (pinned host and device) or cnPrecom is wiped before a stage returns.
#include <sys/random.h>

#include <cstring>
#include <string>
#include <vector>

#include "cz_connect.h"
#include "cz_internal.h"

using namespace czi;

namespace {

enum SlotState : uint8_t { SLOT_FREE, SLOT_EXPECT_WELCOME, SLOT_EXPECT_READY, SLOT_FAILED, SLOT_CONNECTED };

struct Slot {
    SlotState state = SLOT_FREE;
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

uint64_t up16(uint64_t n) { return (n + 15) & ~15ull; }

int fill_random(uint8_t *out, size_t n)
{
    size_t got = 0;
    while (got < n) {
        ssize_t r = getrandom(out + got, n - got, 0);
        if (r < 0)
            return fail(CZ_EINVAL, "cz_connector: getrandom failed");
        got += (size_t)r;
    }
    return CZ_OK;
}

// off[i] + size[i] inside [0, cmds_bytes) for every command
bool commands_inside(uint32_t count, uint64_t cmds_bytes, const uint64_t *off, const uint32_t *size)
{
    for (uint32_t i = 0; i < count; i++)
        if (off[i] > cmds_bytes || size[i] > cmds_bytes - off[i])
            return false;
    return true;
}

}  // namespace

struct cz_connector {
    int device = 0;
    int socket_type = 0;
    uint32_t max_pending = 0;
    uint32_t meta_len = 0;            // the metadata INITIATE carries
    hipStream_t stream = nullptr;
    std::vector<Slot> slots;
    std::vector<int32_t> free_slots;  // handed out from the back
    DevBuf konst;                     // CZC_KONST: the long-term secret c, C, the metadata
    DevBuf state;                     // max_pending x CZC_STATE
    DevBuf work;                      // a stage's jobs, records, scratch and output
    HostBuf h_in, h_out;              // pinned staging of the same
    std::vector<uint32_t> item;       // lane -> index of its command in the caller's batch

    ~cz_connector()
    {
        (void)hipSetDevice(device);
        if (stream) {
            if (konst.ptr)
                (void)hipMemsetAsync(konst.ptr, 0, konst.cap, stream);
            if (state.ptr)
                (void)hipMemsetAsync(state.ptr, 0, state.cap, stream);
            if (work.ptr)
                (void)hipMemsetAsync(work.ptr, 0, work.cap, stream);
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        if (h_in.ptr)
            secure_wipe(h_in.ptr, h_in.cap);
        if (h_out.ptr)
            secure_wipe(h_out.ptr, h_out.cap);
        for (Slot &s : slots)
            s.wipe();
        konst.release();
        state.release();
        work.release();
        h_in.release();
        h_out.release();
    }

    Slot *slot(int32_t id) { return id >= 0 && (uint32_t)id < max_pending ? &slots[(size_t)id] : nullptr; }
    const Slot *slot(int32_t id) const { return id >= 0 && (uint32_t)id < max_pending ? &slots[(size_t)id] : nullptr; }

    void free_slot(int32_t id)
    {
        slots[(size_t)id].wipe();
        free_slots.push_back(id);
    }

    // Wipe what a stage staged (it carried c', kH or cnPrecom), also after an error.
    void wipe_staging(uint64_t dev_bytes, uint64_t in_bytes, uint64_t out_bytes)
    {
        if (work.ptr && dev_bytes)
            (void)hipMemsetAsync(work.ptr, 0, dev_bytes, stream);
        (void)hipStreamSynchronize(stream);
        if (h_in.ptr)
            secure_wipe(h_in.ptr, in_bytes);
        if (h_out.ptr)
            secure_wipe(h_out.ptr, out_bytes);
    }

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
    c->device = device;
    c->socket_type = socket_type;
    c->max_pending = max_pending;
    c->meta_len = (uint32_t)meta.size();
    c->slots.resize(max_pending);
    c->free_slots.reserve(max_pending);
    for (uint32_t i = max_pending; i > 0; i--)
        c->free_slots.push_back((int32_t)(i - 1));
    uint8_t k[CZC_KONST] = {};
    memcpy(k + CZC_KONST_SECRET, secret_key, 32);
    memcpy(k + CZC_KONST_PUBLIC, public_key, 32);
    memcpy(k + CZC_KONST_META, meta.data(), meta.size());
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = c->konst.reserve(sizeof k)) != hipSuccess ||
        (e = c->state.reserve((uint64_t)CZC_STATE * max_pending)) != hipSuccess ||
        (e = hipMemsetAsync(c->state.ptr, 0, c->state.cap, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->konst.ptr, k, sizeof k, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        secure_wipe(k, sizeof k);
        delete c;
        return hip_fail(e, "cz_connector_create");
    }
    secure_wipe(k, sizeof k);
    *out = c;
    return CZ_OK;
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
    auto give_back = [&]() {  // (a failed call hands out no slot; a record a lane may have written is wiped)
        for (uint32_t j = 0; j < nj; j++) {
            if (c->state.ptr)
                (void)hipMemsetAsync((uint8_t *)c->state.ptr + (uint64_t)CZC_STATE * (uint32_t)res[c->item[j]].slot, 0,
                                     CZC_STATE, c->stream);
            c->free_slot(res[c->item[j]].slot);
            res[c->item[j]].slot = -1;
        }
    };
    // 2. one staging block: jobs | records, then the key agreements and the output on the device
    const uint64_t jobs_b = up16(2ull * nj * sizeof(cza_job));
    const uint64_t in_b = jobs_b + (uint64_t)CZC_IN1 * nj;
    const uint64_t x_off = in_b, out_off = x_off + (uint64_t)CZC_X1 * nj;
    const uint64_t out_b = (uint64_t)CZC_OUT1 * nj;
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess || (e = c->work.reserve(out_off + out_b)) != hipSuccess ||
        (e = c->h_in.reserve(in_b)) != hipSuccess || (e = c->h_out.reserve(out_b)) != hipSuccess) {
        give_back();
        return hip_fail(e, "cz_connector_hello: buffers");
    }
    uint8_t *h = (uint8_t *)c->h_in.ptr, *d = (uint8_t *)c->work.ptr;
    cza_job *jobs = (cza_job *)h;  // (every byte the kernels read is written below: no blanket memset)
    int rc = CZ_OK;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = c->item[j];
        uint8_t *r = h + jobs_b + (uint64_t)CZC_IN1 * j;
        memcpy(r + CZC_IN1_SERVER, server_keys + 32ull * i, 32);
        if (test_secrets)
            memcpy(r + CZC_IN1_SECRET, test_secrets + 32ull * i, 32);
        else
            rc = fill_random(r + CZC_IN1_SECRET, 32);
        const int32_t slot = res[i].slot;
        memcpy(r + CZC_IN1_SLOT, &slot, 4);
        memset(r + CZC_IN1_SLOT + 4, 0, CZC_IN1 - CZC_IN1_SLOT - 4);
        const uint8_t *dr = d + jobs_b + (uint64_t)CZC_IN1 * j;
        uint8_t *dx = d + x_off + (uint64_t)CZC_X1 * j;
        jobs[2 * j] = cza_job{dr + CZC_IN1_SECRET, nullptr, dx, nullptr, CZA_JOB_BASE, 0};                           // C'
        jobs[2 * j + 1] = cza_job{dr + CZC_IN1_SECRET, dr + CZC_IN1_SERVER, dx + 32, nullptr, CZA_JOB_BEFORENM, 0};  // kH
    }
    if (rc != CZ_OK) {
        secure_wipe(h, in_b);
        give_back();
        return rc;
    }
    // 3. the launch chain and its one synchronisation
    if ((e = hipMemsetAsync(d + out_off, 0xff, out_b, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(d, h, in_b, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = czk_x25519_jobs((const cza_job *)d, 2 * nj, c->stream)) != hipSuccess ||
        (e = czk_con_hello(d + jobs_b, d + x_off, d + out_off, c->state.ptr, nj, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->h_out.ptr, d + out_off, out_b, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(d, 0, out_off, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->wipe_staging(out_off + out_b, in_b, out_b);
        give_back();
        return hip_fail(e, "cz_connector_hello");
    }
    for (uint32_t j = 0; j < nj; j++)  // the staged secret: c' (the rest is public)
        secure_wipe(h + jobs_b + (uint64_t)CZC_IN1 * j + CZC_IN1_SECRET, 32);
    // 4. results: the HELLO and a slot that waits for its WELCOME
    const uint8_t *ho = (const uint8_t *)c->h_out.ptr;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = ho + (uint64_t)CZC_OUT1 * j;
        uint32_t st;
        memcpy(&st, o + CZC_OUT1_STATUS, 4);
        if (st == CZA_ST_OK) {
            Slot &s = c->slots[(size_t)res[i].slot];
            memcpy(reply + reply_stride * i, o + CZC_OUT1_CMD, 200);
            res[i].reply_len = 200;
            memcpy(s.server_key, server_keys + 32ull * i, 32);
            memcpy(s.cn_public, o + CZC_OUT1_CMD + 80, 32);
            s.state = SLOT_EXPECT_WELCOME;
        } else {  // the lane did not run: a device failure the runtime did not report
            (void)hipMemsetAsync((uint8_t *)c->state.ptr + (uint64_t)CZC_STATE * (uint32_t)res[i].slot, 0, CZC_STATE,
                                 c->stream);
            c->free_slot(res[i].slot);
            res[i].slot = -1;
            res[i].rc = CZ_EHIP;
            rc = fail(CZ_EHIP, "cz_connector_hello: lane %u left no status", j);
        }
    }
    return rc;
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
    const uint64_t jobs_b = up16(2ull * nj * sizeof(cza_job));
    const uint64_t in_b = jobs_b + (uint64_t)CZC_IN2 * nj;
    const uint64_t x_off = in_b, out_off = x_off + (uint64_t)CZC_X2 * nj;
    const uint64_t out_b = (uint64_t)CZC_OUT2 * nj;
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess || (e = c->work.reserve(out_off + out_b)) != hipSuccess ||
        (e = c->h_in.reserve(in_b)) != hipSuccess || (e = c->h_out.reserve(out_b)) != hipSuccess)
        return hip_fail(e, "cz_connector_welcome: buffers");
    uint8_t *h = (uint8_t *)c->h_in.ptr, *d = (uint8_t *)c->work.ptr;
    uint8_t *d_state = (uint8_t *)c->state.ptr;
    const uint8_t *d_konst = (const uint8_t *)c->konst.ptr;
    cza_job *jobs = (cza_job *)h;  // (every byte the kernels read is written below: no blanket memset)
    int rc = CZ_OK;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *m = cmds + off[i];
        const Slot &s = c->slots[(size_t)slot[i]];
        uint8_t *r = h + jobs_b + (uint64_t)CZC_IN2 * j;
        memset(r, 0, CZC_IN2_NONCE);
        memcpy(r + CZC_IN2_SLOT, &slot[i], 4);
        memcpy(r + CZC_IN2_NONCE, m + 8, 16);
        memcpy(r + CZC_IN2_BOX, m + 24, 144);
        memcpy(r + CZC_IN2_SERVER, s.server_key, 32);
        memcpy(r + CZC_IN2_CP, s.cn_public, 32);
        if (test_entropy)
            memcpy(r + CZC_IN2_VNONCE, test_entropy + 16ull * i, 16);
        else
            rc = fill_random(r + CZC_IN2_VNONCE, 16);
        uint8_t *st = d_state + (uint64_t)CZC_STATE * (uint32_t)slot[i];
        const uint8_t *sp = d + x_off + (uint64_t)CZC_X2 * j + CZC_X2_SP;
        const uint32_t *gate = (const uint32_t *)(d + out_off + (uint64_t)CZC_OUT2 * j + CZC_OUT2_STATUS);
        // once 2a has opened the box that holds S': the session key and the vouch's key, into the slot
        jobs[2 * j] = cza_job{st + CZC_STATE_SECRET, sp, st + CZC_STATE_PRECOM, gate, CZA_JOB_BEFORENM, 0};
        jobs[2 * j + 1] = cza_job{d_konst + CZC_KONST_SECRET, sp, st + CZC_STATE_KV, gate, CZA_JOB_BEFORENM, 0};
    }
    if (rc != CZ_OK)
        return rc;
    if ((e = hipMemsetAsync(d + out_off, 0xff, out_b, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(d, h, in_b, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = czk_con_welcome(d + jobs_b, d + out_off, d + x_off, d_state, nj, c->stream)) != hipSuccess ||
        (e = czk_x25519_jobs((const cza_job *)d, 2 * nj, c->stream)) != hipSuccess ||
        (e = czk_con_initiate(d + out_off, d + x_off, d + jobs_b, d_state, d_konst, c->meta_len, nj, c->stream)) !=
            hipSuccess ||
        (e = hipMemcpyAsync(c->h_out.ptr, d + out_off, out_b, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(d, 0, out_off + out_b, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->wipe_staging(out_off + out_b, in_b, out_b);
        return hip_fail(e, "cz_connector_welcome");
    }
    // 2. results: the INITIATE and a slot that waits for its READY
    // (this stage stages no secret through the host: the keys went from the ladder into the slot table)
    const uint8_t *ho = (const uint8_t *)c->h_out.ptr;
    const uint32_t init_len = 113 + 16 + 128 + c->meta_len;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = ho + (uint64_t)CZC_OUT2 * j;
        uint32_t st;
        memcpy(&st, o + CZC_OUT2_STATUS, 4);
        if (st == CZA_ST_OK) {
            memcpy(reply + reply_stride * i, o + CZC_OUT2_CMD, init_len);
            res[i].reply_len = init_len;
            c->slots[(size_t)slot[i]].state = SLOT_EXPECT_READY;
        } else if (st == CZA_ST_CRYPTO) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
        } else {  // the lane did not run: a device failure the runtime did not report
            res[i].rc = CZ_EHIP;
            rc = fail(CZ_EHIP, "cz_connector_welcome: lane %u left no status", j);
        }
    }
    return rc;
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
    const uint64_t in_b = (uint64_t)CZC_IN3 * nj;
    const uint64_t out_off = in_b, out_b = (uint64_t)CZC_OUT3 * nj;
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess || (e = c->work.reserve(out_off + out_b)) != hipSuccess ||
        (e = c->h_in.reserve(in_b)) != hipSuccess || (e = c->h_out.reserve(out_b)) != hipSuccess)
        return hip_fail(e, "cz_connector_ready: buffers");
    uint8_t *h = (uint8_t *)c->h_in.ptr, *d = (uint8_t *)c->work.ptr;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = h + (uint64_t)CZC_IN3 * j;
        const uint32_t plain_len = size[i] - 14 - 16;  // 0 .. CZC_READY_MAX
        memcpy(r + CZC_IN3_SLOT, &slot[i], 4);
        memcpy(r + CZC_IN3_LEN, &plain_len, 4);
        memcpy(r + CZC_IN3_NONCE, m + 6, 8);
        memcpy(r + CZC_IN3_BOX, m + 14, size[i] - 14);
        memset(r + CZC_IN3_BOX + 16 + plain_len, 0, (0u - plain_len) & 15u);  // the last chunk's pad
    }
    if ((e = hipMemsetAsync(d + out_off, 0xff, out_b, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(d, h, in_b, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
        (e = czk_con_ready(d, d + out_off, c->state.ptr, nj, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(c->h_out.ptr, d + out_off, out_b, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(d, 0, out_off + out_b, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess) {
        c->wipe_staging(out_off + out_b, in_b, out_b);
        return hip_fail(e, "cz_connector_ready");
    }
    // 2. results: the metadata (Metadata.read + the Socket-Type check) on the host, then the session
    int rc = CZ_OK;
    const uint8_t *ho = (const uint8_t *)c->h_out.ptr;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = c->item[j];
        const uint8_t *o = ho + (uint64_t)CZC_OUT3 * j;
        Slot &s = c->slots[(size_t)slot[i]];
        uint32_t st;
        memcpy(&st, o + CZC_OUT3_STATUS, 4);
        if (st == CZA_ST_CRYPTO) {
            res[i].rc = CZ_EPROTO;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
            continue;
        }
        if (st != CZA_ST_OK) {  // the lane did not run: a device failure the runtime did not report
            res[i].rc = CZ_EHIP;
            rc = fail(CZ_EHIP, "cz_connector_ready: lane %u left no status", j);
            continue;
        }
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
    secure_wipe(c->h_out.ptr, out_b);  // it held cnPrecom
    return rc;
}

int cz_connector_session(const cz_connector *c, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                         uint64_t *cn_peer_nonce)
{
    if (!c || !precom || !cn_nonce || !cn_peer_nonce)
        return fail(CZ_EINVAL, "cz_connector_session: null pointer");
    const Slot *s = c->slot(slot);
    if (!s || s->state != SLOT_CONNECTED)
        return fail(CZ_EINVAL, "cz_connector_session: slot %d has no completed handshake", slot);
    memcpy(precom, s->precom, 32);
    *cn_nonce = 3;  // HELLO took 1, INITIATE 2
    *cn_peer_nonce = s->peer_nonce;
    return CZ_OK;
}

int cz_connector_peer_property(const cz_connector *c, int32_t slot, const char *name, const uint8_t **value,
                               uint32_t *len)
{
    if (!c || !name || !value || !len)
        return fail(CZ_EINVAL, "cz_connector_peer_property: null pointer");
    const Slot *s = c->slot(slot);
    if (s && s->state != SLOT_FREE)
        for (const auto &p : s->peer)
            if (p.first == name) {
                *value = p.second.data();
                *len = (uint32_t)p.second.size();
                return CZ_OK;
            }
    return fail(CZ_EINVAL, "cz_connector_peer_property: no property %s on slot %d", name, slot);
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
    uint8_t k[32];
    uint64_t n, pn;
    int rc = cz_connector_session(c, slot, k, &n, &pn);
    if (rc != CZ_OK)
        return rc;
    rc = cz_engine_add_conn(e, 0, k, n, pn);
    secure_wipe(k, 32);
    return rc;
}

int cz_connector_release(cz_connector *c, int32_t slot)
{
    Slot *s = c ? c->slot(slot) : nullptr;
    if (!s || s->state == SLOT_FREE)
        return fail(CZ_EINVAL, "cz_connector_release: slot %d is not in use", slot);
    // the device record (c', kH, cnPrecom, kV): wiped in stream order, so before any later stage can
    // hand the slot to another connection; cz_connector_destroy waits for it
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess ||
        (e = hipMemsetAsync((uint8_t *)c->state.ptr + (uint64_t)CZC_STATE * (uint32_t)slot, 0, CZC_STATE, c->stream)) !=
            hipSuccess)
        return hip_fail(e, "cz_connector_release");
    c->free_slot(slot);
    return CZ_OK;
}

uint32_t cz_connector_pending(const cz_connector *c)
{
    return c ? c->max_pending - (uint32_t)c->free_slots.size() : 0;
}

}  // extern "C"
