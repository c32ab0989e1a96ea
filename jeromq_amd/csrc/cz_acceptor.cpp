// cz_acceptor.cpp -- the server half of the CURVE handshake for many connections at once (section 11
// of the header): N HELLO commands -> N WELCOME commands, N INITIATE commands -> N READY commands,
// each stage a fixed chain of device work whatever N is, ending in sessions cz_engine takes.
//
// Mirrors CurveServerMechanism.processHello :254-299, produceWelcome :301-358, processInitiate
// :360-471, produceReady :473-507 and produceError :509-517 item by item (no ZAP handler configured);
// the per-connection form of the same state machine is cz_curve_hs.cpp, whose metadata parser and
// Socket-Type table this file shares (cz_internal.h).
//
// Launch chain (one stream, one synchronisation per stage):
//   stage 1: memset out | H2D jobs + records | k_x25519_jobs (3 lanes per connection: S' = s'.9,
//            k1 = beforenm(C', s), cnPrecom = beforenm(C', s')) | k_acc_welcome | D2H out | wipe | sync
//   stage 2: memset out | H2D jobs + records | k_acc_initiate | k_x25519_jobs (k3 = beforenm(C, s'),
//            gated on 2a's status) | k_acc_ready | D2H out | wipe | sync
// k1 serves the HELLO open and the WELCOME box; cnPrecom is computed in stage 1 so that stage 2 has
// one ladder on its critical path, not two ("Batched server handshake").  No key agreement runs twice for
// a connection.  The host side parses command framing before the launch and the metadata after it.
//
// Secrets: s', the cookie key and cnPrecom live in the device state table, indexed by slot, until
// cz_acceptor_release / destroy wipes the record.  The staging that carried them (pinned host and
// device, both directions) is wiped before a stage returns.  The cookie plaintext never leaves the
// device's registers.
#include <sys/random.h>

#include <cstring>
#include <string>
#include <vector>

#include "cz_accept.h"
#include "cz_internal.h"

using namespace czi;

namespace {

enum SlotState : uint8_t { SLOT_FREE, SLOT_EXPECT_INITIATE, SLOT_FAILED, SLOT_CONNECTED };

struct Slot {
    SlotState state = SLOT_FREE;
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

uint64_t up16(uint64_t n) { return (n + 15) & ~15ull; }

int fill_random(uint8_t *out, size_t n)
{
    size_t got = 0;
    while (got < n) {
        ssize_t r = getrandom(out + got, n - got, 0);
        if (r < 0)
            return fail(CZ_EINVAL, "cz_acceptor: getrandom failed");
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

struct cz_acceptor {
    int device = 0;
    int socket_type = 0;
    uint32_t max_pending = 0;
    hipStream_t stream = nullptr;
    std::vector<Slot> slots;
    std::vector<int32_t> free_slots;  // handed out from the back
    std::vector<uint8_t> meta;        // the metadata READY carries
    DevBuf konst;                     // [0,32) the long-term secret s, [32, 32 + CZA_META_MAX) metadata
    DevBuf state;                     // max_pending x CZA_STATE
    DevBuf work;                      // a stage's jobs, records, key agreements and output
    HostBuf h_in, h_out;              // pinned staging of the same
    std::vector<uint32_t> item;       // lane -> index of its command in the caller's batch

    ~cz_acceptor()
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

    // Wipe what a stage staged (it carried s', cookie keys, k1, cnPrecom), also after an error.
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
    a->device = device;
    a->socket_type = socket_type;
    a->max_pending = max_pending;
    a->meta = std::move(meta);
    a->slots.resize(max_pending);
    a->free_slots.reserve(max_pending);
    for (uint32_t i = max_pending; i > 0; i--)
        a->free_slots.push_back((int32_t)(i - 1));
    uint8_t k[32 + CZA_META_MAX] = {};
    memcpy(k, secret_key, 32);
    memcpy(k + 32, a->meta.data(), a->meta.size());
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = a->konst.reserve(sizeof k)) != hipSuccess ||
        (e = a->state.reserve((uint64_t)CZA_STATE * max_pending)) != hipSuccess ||
        (e = hipMemsetAsync(a->state.ptr, 0, a->state.cap, a->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(a->konst.ptr, k, sizeof k, hipMemcpyHostToDevice, a->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(a->stream)) != hipSuccess) {
        secure_wipe(k, sizeof k);
        delete a;
        return hip_fail(e, "cz_acceptor_create");
    }
    secure_wipe(k, sizeof k);
    *out = a;
    return CZ_OK;
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
    auto give_back = [&]() {  // (a failed call hands out no slot; a record a lane may have written is wiped)
        for (uint32_t j = 0; j < nj; j++) {
            if (a->state.ptr)
                (void)hipMemsetAsync((uint8_t *)a->state.ptr + (uint64_t)CZA_STATE * (uint32_t)res[a->item[j]].slot, 0,
                                     CZA_STATE, a->stream);
            a->free_slot(res[a->item[j]].slot);
            res[a->item[j]].slot = -1;
        }
    };
    // 2. one staging block: jobs | records, then the key agreements and the output on the device
    const uint64_t jobs_b = up16(3ull * nj * sizeof(cza_job));
    const uint64_t in_b = jobs_b + (uint64_t)CZA_IN1 * nj;
    const uint64_t x_off = in_b, out_off = x_off + (uint64_t)CZA_X1 * nj;
    const uint64_t out_b = (uint64_t)CZA_OUT1 * nj;
    hipError_t e;
    if ((e = hipSetDevice(a->device)) != hipSuccess || (e = a->work.reserve(out_off + out_b)) != hipSuccess ||
        (e = a->h_in.reserve(in_b)) != hipSuccess || (e = a->h_out.reserve(out_b)) != hipSuccess) {
        give_back();
        return hip_fail(e, "cz_acceptor_hello: buffers");
    }
    uint8_t *h = (uint8_t *)a->h_in.ptr, *d = (uint8_t *)a->work.ptr;
    const uint8_t *d_key = (const uint8_t *)a->konst.ptr;
    cza_job *jobs = (cza_job *)h;  // (every byte the kernels read is written below: no blanket memset)
    int rc = CZ_OK;
    for (uint32_t j = 0; j < nj && rc == CZ_OK; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = h + jobs_b + (uint64_t)CZA_IN1 * j;
        memcpy(r + CZA_IN1_CP, m + 80, 32);
        memcpy(r + CZA_IN1_NONCE, m + 112, 8);
        memcpy(r + CZA_IN1_BOX, m + 120, 80);
        static_assert(CZA_IN1_SECRET == CZA_IN1_ENTROPY + 64, "entropy and s' are drawn in one call");
        if (!test_entropy && !test_secrets) {
            rc = fill_random(r + CZA_IN1_ENTROPY, 96);
        } else {
            if (test_entropy)
                memcpy(r + CZA_IN1_ENTROPY, test_entropy + 64ull * i, 64);
            else
                rc = fill_random(r + CZA_IN1_ENTROPY, 64);
            if (test_secrets)
                memcpy(r + CZA_IN1_SECRET, test_secrets + 32ull * i, 32);
            else if (rc == CZ_OK)
                rc = fill_random(r + CZA_IN1_SECRET, 32);
        }
        const int32_t slot = res[i].slot;
        memcpy(r + CZA_IN1_SLOT, &slot, 4);
        const uint8_t *dr = d + jobs_b + (uint64_t)CZA_IN1 * j;
        uint8_t *dx = d + x_off + (uint64_t)CZA_X1 * j;
        jobs[3 * j] = cza_job{dr + CZA_IN1_SECRET, nullptr, dx, nullptr, CZA_JOB_BASE, 0};                    // S'
        jobs[3 * j + 1] = cza_job{d_key, dr + CZA_IN1_CP, dx + 32, nullptr, CZA_JOB_BEFORENM, 0};             // k1
        jobs[3 * j + 2] = cza_job{dr + CZA_IN1_SECRET, dr + CZA_IN1_CP, dx + 64, nullptr, CZA_JOB_BEFORENM, 0};  // cnPrecom
    }
    if (rc != CZ_OK) {
        secure_wipe(h, in_b);
        give_back();
        return rc;
    }
    // 3. the launch chain and its one synchronisation
    if ((e = hipMemsetAsync(d + out_off, 0xff, out_b, a->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(d, h, in_b, hipMemcpyHostToDevice, a->stream)) != hipSuccess ||
        (e = czk_x25519_jobs((const cza_job *)d, 3 * nj, a->stream)) != hipSuccess ||
        (e = czk_acc_welcome(d + jobs_b, d + x_off, d + out_off, a->state.ptr, nj, a->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(a->h_out.ptr, d + out_off, out_b, hipMemcpyDeviceToHost, a->stream)) != hipSuccess ||
        (e = hipMemsetAsync(d, 0, out_off, a->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(a->stream)) != hipSuccess) {
        a->wipe_staging(out_off + out_b, in_b, out_b);
        give_back();
        return hip_fail(e, "cz_acceptor_hello");
    }
    for (uint32_t j = 0; j < nj; j++)  // the staged secrets: cookie key and s' (the rest came off the wire)
        secure_wipe(h + jobs_b + (uint64_t)CZA_IN1 * j + CZA_IN1_ENTROPY, 96);
    // 4. results: WELCOME and a pending slot, or ERROR (processHello's failed open, produceError)
    const uint8_t *ho = (const uint8_t *)a->h_out.ptr;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *o = ho + (uint64_t)CZA_OUT1 * j;
        uint32_t st;
        memcpy(&st, o + CZA_OUT1_STATUS, 4);
        uint8_t *rp = reply + reply_stride * i;
        if (st == CZA_ST_OK) {
            memcpy(rp, o + CZA_OUT1_CMD, 168);
            res[i].reply_len = 168;
            a->slots[(size_t)res[i].slot].state = SLOT_EXPECT_INITIATE;
        } else if (st == CZA_ST_CRYPTO) {
            memcpy(rp, "\x05" "ERROR\x00", 7);
            res[i].reply_len = 7;
            res[i].event = CZ_ZMTP_CRYPTOGRAPHIC;
            a->free_slot(res[i].slot);
            res[i].slot = -1;
        } else {  // the lane did not run: a device failure the runtime did not report
            a->free_slot(res[i].slot);
            res[i].slot = -1;
            res[i].rc = CZ_EHIP;
            rc = fail(CZ_EHIP, "cz_acceptor_hello: lane %u left no status", j);
        }
    }
    return rc;
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
    const uint64_t jobs_b = up16((uint64_t)nj * sizeof(cza_job));
    const uint64_t in_b = jobs_b + (uint64_t)CZA_IN2 * nj;
    const uint64_t x_off = in_b, out_off = x_off + 32ull * nj;
    const uint64_t out_b = (uint64_t)CZA_OUT2 * nj;
    hipError_t e;
    if ((e = hipSetDevice(a->device)) != hipSuccess || (e = a->work.reserve(out_off + out_b)) != hipSuccess ||
        (e = a->h_in.reserve(in_b)) != hipSuccess || (e = a->h_out.reserve(out_b)) != hipSuccess)
        return hip_fail(e, "cz_acceptor_initiate: buffers");
    uint8_t *h = (uint8_t *)a->h_in.ptr, *d = (uint8_t *)a->work.ptr;
    const uint8_t *d_state = (const uint8_t *)a->state.ptr;
    cza_job *jobs = (cza_job *)h;  // (every byte the kernels read is written below: no blanket memset)
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *m = cmds + off[i];
        uint8_t *r = h + jobs_b + (uint64_t)CZA_IN2 * j;
        const uint32_t plain_len = size[i] - 113 - 16;  // 128 .. CZA_INIT_MAX
        memcpy(r + CZA_IN2_SLOT, &slot[i], 4);
        memcpy(r + CZA_IN2_LEN, &plain_len, 4);
        memcpy(r + CZA_IN2_NONCE, m + 105, 8);
        memcpy(r + CZA_IN2_COOKIE_NONCE, m + 9, 16);
        memcpy(r + CZA_IN2_COOKIE, m + 25, 80);
        memcpy(r + CZA_IN2_BOX, m + 113, size[i] - 113);
        memset(r + CZA_IN2_BOX + 16 + plain_len, 0, (0u - plain_len) & 15u);  // the last chunk's pad
        uint8_t *dout = d + out_off + (uint64_t)CZA_OUT2 * j;
        // k3 = beforenm(C, s'): the vouch's key, once 2a has opened the box that holds C
        jobs[j] = cza_job{d_state + (uint64_t)CZA_STATE * (uint32_t)slot[i] + CZA_STATE_SECRET, dout + CZA_OUT2_PLAIN,
                          d + x_off + 32ull * j, (const uint32_t *)(dout + CZA_OUT2_STATUS), CZA_JOB_BEFORENM, 0};
    }
    if ((e = hipMemsetAsync(d + out_off, 0xff, out_b, a->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(d, h, in_b, hipMemcpyHostToDevice, a->stream)) != hipSuccess ||
        (e = czk_acc_initiate(d + jobs_b, d + out_off, d_state, nj, a->stream)) != hipSuccess ||
        (e = czk_x25519_jobs((const cza_job *)d, nj, a->stream)) != hipSuccess ||
        (e = czk_acc_ready(d + out_off, d + x_off, d + jobs_b, d_state, (const uint8_t *)a->konst.ptr + 32,
                           (uint32_t)a->meta.size(), nj, a->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(a->h_out.ptr, d + out_off, out_b, hipMemcpyDeviceToHost, a->stream)) != hipSuccess ||
        (e = hipMemsetAsync(d, 0, out_off + out_b, a->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(a->stream)) != hipSuccess) {
        a->wipe_staging(out_off + out_b, in_b, out_b);
        return hip_fail(e, "cz_acceptor_initiate");
    }
    // 2. results: the metadata (Metadata.read + the Socket-Type check) on the host, then READY
    int rc = CZ_OK;
    const uint8_t *ho = (const uint8_t *)a->h_out.ptr;
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = a->item[j];
        const uint8_t *o = ho + (uint64_t)CZA_OUT2 * j;
        Slot &s = a->slots[(size_t)slot[i]];
        uint32_t st;
        memcpy(&st, o + CZA_OUT2_STATUS, 4);
        if (st == CZA_ST_CRYPTO || st == CZA_ST_KEY_EXCHANGE) {
            res[i].rc = CZ_EPROTO;
            res[i].event = st == CZA_ST_KEY_EXCHANGE ? CZ_ZMTP_KEY_EXCHANGE : CZ_ZMTP_CRYPTOGRAPHIC;
            continue;
        }
        if (st != CZA_ST_OK) {  // the lane did not run: a device failure the runtime did not report
            res[i].rc = CZ_EHIP;
            rc = fail(CZ_EHIP, "cz_acceptor_initiate: lane %u left no status", j);
            continue;
        }
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
        secure_wipe((uint8_t *)a->h_out.ptr + (uint64_t)CZA_OUT2 * j + CZA_OUT2_PRECOM, 32);
        s.peer_nonce = get_be64(m + 105);
        s.state = SLOT_CONNECTED;
        uint8_t *rp = reply + reply_stride * i;
        memcpy(rp, "\x05READY", 6);
        put_be64(rp + 6, 1);  // cn_nonce = 1; the session continues at 2
        memcpy(rp + 14, o + CZA_OUT2_READY, 16 + a->meta.size());
        res[i].reply_len = (uint32_t)(14 + 16 + a->meta.size());
    }
    // (stage 2 stages no secret towards the device; what came back held cnPrecom, wiped above, and
    // for lanes whose metadata failed, wiped here)
    for (uint32_t j = 0; j < nj; j++)
        if (a->slots[(size_t)slot[a->item[j]]].state != SLOT_CONNECTED)
            secure_wipe((uint8_t *)a->h_out.ptr + (uint64_t)CZA_OUT2 * j + CZA_OUT2_PRECOM, 32);
    return rc;
}

int cz_acceptor_session(const cz_acceptor *a, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                        uint64_t *cn_peer_nonce)
{
    if (!a || !precom || !cn_nonce || !cn_peer_nonce)
        return fail(CZ_EINVAL, "cz_acceptor_session: null pointer");
    const Slot *s = a->slot(slot);
    if (!s || s->state != SLOT_CONNECTED)
        return fail(CZ_EINVAL, "cz_acceptor_session: slot %d has no completed handshake", slot);
    memcpy(precom, s->precom, 32);
    *cn_nonce = 2;
    *cn_peer_nonce = s->peer_nonce;
    return CZ_OK;
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
    if (!a || !name || !value || !len)
        return fail(CZ_EINVAL, "cz_acceptor_peer_property: null pointer");
    const Slot *s = a->slot(slot);
    if (s && s->state != SLOT_FREE)
        for (const auto &p : s->peer)
            if (p.first == name) {
                *value = p.second.data();
                *len = (uint32_t)p.second.size();
                return CZ_OK;
            }
    return fail(CZ_EINVAL, "cz_acceptor_peer_property: no property %s on slot %d", name, slot);
}

int cz_engine_add_accepted(cz_engine *e, const cz_acceptor *a, int32_t slot)
{
    uint8_t k[32];
    uint64_t n, pn;
    int rc = cz_acceptor_session(a, slot, k, &n, &pn);
    if (rc != CZ_OK)
        return rc;
    rc = cz_engine_add_conn(e, 1, k, n, pn);
    secure_wipe(k, 32);
    return rc;
}

int cz_acceptor_release(cz_acceptor *a, int32_t slot)
{
    Slot *s = a ? a->slot(slot) : nullptr;
    if (!s || s->state == SLOT_FREE)
        return fail(CZ_EINVAL, "cz_acceptor_release: slot %d is not in use", slot);
    // the device record (s', cookie key, cnPrecom): wiped in stream order, so before any later stage
    // can hand the slot to another connection; cz_acceptor_destroy waits for it
    hipError_t e;
    if ((e = hipSetDevice(a->device)) != hipSuccess ||
        (e = hipMemsetAsync((uint8_t *)a->state.ptr + (uint64_t)CZA_STATE * (uint32_t)slot, 0, CZA_STATE, a->stream)) !=
            hipSuccess)
        return hip_fail(e, "cz_acceptor_release");
    a->free_slot(slot);
    return CZ_OK;
}

uint32_t cz_acceptor_pending(const cz_acceptor *a)
{
    return a ? a->max_pending - (uint32_t)a->free_slots.size() : 0;
}

}  // extern "C"
