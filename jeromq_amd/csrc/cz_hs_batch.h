// cz_hs_batch.h -- the host core of the two batched CURVE handshakes (cz_acceptor.cpp, cz_connector.cpp):
// the handle (slot table, device buffers, pinned staging), the shape every stage has, and the entry
// points that are the same on both sides.  What differs between the sides comes in as values: the name
// used in messages, the size of a slot's device record, the constants copied to the device.
//
// Every stage is one staging block and one chain on one stream with one synchronisation:
//   device:  jobs | input records | x (key agreements, scratch) | output records
//   chain:   memset out 0xff | H2D jobs + records | the stage's kernels | D2H out | wipe | sync
// The memset makes a lane that never ran visible (CZA_ST_NOT_RUN); the wipe zeroes the device staging
// behind the kernels.  Stage lays the block out, runs the chain and cleans up after a failure, so a
// stage function is its framing checks, the filling of its records and job descriptors, its kernel
// launches and what it does with each lane's status.
#pragma once
#include <sys/random.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "cz_hs_records.h"
#include "cz_internal.h"
#include "cz_session.h"

namespace czi {

inline uint64_t up16(uint64_t n) { return (n + 15) & ~15ull; }

// n bytes from the kernel's generator; `who` names the caller in the message
inline int fill_random(uint8_t *out, size_t n, const char *who)
{
    size_t got = 0;
    while (got < n) {
        ssize_t r = getrandom(out + got, n - got, 0);
        if (r < 0)
            return fail(CZ_EINVAL, "%s: getrandom failed", who);
        got += (size_t)r;
    }
    return CZ_OK;
}

// off[i] + size[i] inside [0, cmds_bytes) for every command
inline bool commands_inside(uint32_t count, uint64_t cmds_bytes, const uint64_t *off, const uint32_t *size)
{
    for (uint32_t i = 0; i < count; i++)
        if (off[i] > cmds_bytes || size[i] > cmds_bytes - off[i])
            return false;
    return true;
}

// A slot is FREE, then in one of its side's waiting states (numbered from SLOT_WAITING), then CONNECTED;
// FAILED from any of them.  Every slot named in a stage leaves the state it was in, going to FAILED,
// before anything else happens to it: a slot named twice in one batch is taken by the first item.
enum : uint8_t { SLOT_FREE, SLOT_FAILED, SLOT_CONNECTED, SLOT_WAITING };

// Slot is the side's host record of a slot.  The core uses its state, precom (cnPrecom, once CONNECTED),
// peer_nonce, peer (the peer's metadata) and wipe(), which leaves it FREE; the rest is the side's own.
template <class Slot>
struct HsBatch {
    const char *const name;     // "cz_acceptor" / "cz_connector"
    const uint32_t state_size;  // bytes of one slot's record in `state`
    int device = 0;
    int socket_type = 0;
    uint32_t max_pending = 0;
    hipStream_t stream = nullptr;
    std::vector<Slot> slots;
    std::vector<int32_t> free_slots;  // handed out from the back
    DevBuf konst;                     // the side's long-term keys and metadata
    DevBuf state;                     // max_pending x state_size: the secrets a connection has between stages
    DevBuf work;                      // a stage's jobs, records, key agreements and output
    HostBuf h_in, h_out;              // pinned staging of the same
    std::vector<uint32_t> item;       // lane -> index of its command in the caller's batch
    DevBuf d_rel;                     // hs_release_batch: the slots whose records one launch wipes
    HostBuf h_rel;                    // pinned staging of the same

    HsBatch(const char *name, uint32_t state_size) : name(name), state_size(state_size) {}
    HsBatch(const HsBatch &) = delete;

    ~HsBatch()
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
        d_rel.release();
        h_rel.release();
    }

    Slot *slot(int32_t id) { return id >= 0 && (uint32_t)id < max_pending ? &slots[(size_t)id] : nullptr; }
    const Slot *slot(int32_t id) const { return id >= 0 && (uint32_t)id < max_pending ? &slots[(size_t)id] : nullptr; }

    void free_slot(int32_t id)
    {
        slots[(size_t)id].wipe();
        free_slots.push_back(id);
    }

    // The slot's device record, wiped in stream order: before any later stage can hand the slot to
    // another connection.  The destructor waits for it.
    hipError_t wipe_record(int32_t id)
    {
        if (!state.ptr)
            return hipSuccess;
        return hipMemsetAsync((uint8_t *)state.ptr + (uint64_t)state_size * (uint32_t)id, 0, state_size, stream);
    }

    // A failed call hands out no slot: the slots of res[item[0 .. nj)] go back to the free list, and a
    // record a lane may have written is wiped.
    void give_back(cz_accept_result *res, uint32_t nj)
    {
        for (uint32_t j = 0; j < nj; j++) {
            int32_t &id = res[item[j]].slot;
            (void)wipe_record(id);
            free_slot(id);
            id = -1;
        }
    }

    // Wipe what a stage staged (short-term secrets, cookie keys, the keys agreed, cnPrecom), also after
    // an error.
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

// The device half of *_create, after the argument checks: the free list, the stream, the slot table
// and the constants k[0 .. k_len), whose copy on the caller's stack is wiped on both paths.  Takes
// ownership of h.
template <class Handle>
int hs_create(Handle **out, Handle *h, const char *where, uint8_t *k, size_t k_len, int socket_type,
              uint32_t max_pending, int device)
{
    h->device = device;
    h->socket_type = socket_type;
    h->max_pending = max_pending;
    h->slots.resize(max_pending);
    h->free_slots.reserve(max_pending);
    for (uint32_t i = max_pending; i > 0; i--)
        h->free_slots.push_back((int32_t)(i - 1));
    hipError_t e;
    const bool failed = (e = hipSetDevice(device)) != hipSuccess ||
                        (e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
                        (e = h->konst.reserve(k_len)) != hipSuccess ||
                        (e = h->state.reserve((uint64_t)h->state_size * max_pending)) != hipSuccess ||
                        (e = hipMemsetAsync(h->state.ptr, 0, h->state.cap, h->stream)) != hipSuccess ||
                        (e = hipMemcpyAsync(h->konst.ptr, k, k_len, hipMemcpyHostToDevice, h->stream)) != hipSuccess ||
                        (e = hipStreamSynchronize(h->stream)) != hipSuccess;
    secure_wipe(k, k_len);
    if (failed) {
        delete h;
        return hip_fail(e, where);
    }
    *out = h;
    return CZ_OK;
}

// cn_nonce: the next nonce the side sends under (the commands it made took the ones before)
template <class Slot>
int hs_session(const HsBatch<Slot> *b, const char *where, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
               uint64_t *cn_peer_nonce, uint64_t next_nonce)
{
    if (!b || !precom || !cn_nonce || !cn_peer_nonce)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    const Slot *s = b->slot(slot);
    if (!s || s->state != SLOT_CONNECTED)
        return fail(CZ_EINVAL, "%s: slot %d has no completed handshake", where, slot);
    memcpy(precom, s->precom, 32);
    *cn_nonce = next_nonce;
    *cn_peer_nonce = s->peer_nonce;
    return CZ_OK;
}

// the session of a CONNECTED slot as a connection of the batching engine
template <class Slot>
int hs_engine_add(cz_engine *e, const HsBatch<Slot> *b, const char *session_name, int32_t slot, uint64_t next_nonce,
                  int server)
{
    uint8_t k[32];
    uint64_t n, pn;
    int rc = hs_session(b, session_name, slot, k, &n, &pn, next_nonce);
    if (rc != CZ_OK)
        return rc;
    rc = cz_engine_add_conn(e, server, k, n, pn);
    secure_wipe(k, 32);
    return rc;
}

// The sessions of `count` slots as connections of the batching engine in one device chain
// (engine_add_sessions, cz_engine.cpp).  cnPrecom never leaves the device: it lies in the slot's
// record of `state`, at precom_off, from the stage that agreed it until the slot is released, and
// k_session_subkeys reads it there.  The stage that made the slot CONNECTED has synchronised the
// handshake's stream, so the engine's stream may read the record; this call returns after the engine's
// synchronisation, so a release issued afterwards on the handshake's stream cannot overtake the read.
// A handshake on another device than the engine has no record the engine's kernels can address: the
// host slot table's precom is staged as cz_engine_add_conns stages its keys (that branch needs two
// GPUs and is not covered by the single-GPU tests).  A slot that is out of range or not CONNECTED
// gives ids[i] = CZ_EINVAL and consumes no id.
template <class Slot>
int hs_engine_add_batch(cz_engine *e, const HsBatch<Slot> *b, const char *where, uint32_t count, const int32_t *slots,
                        int32_t *ids, uint32_t precom_off, uint64_t next_nonce, int server)
{
    if (!e || !b)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    if (count == 0)
        return CZ_OK;
    for (uint32_t i = 0; ids && i < count; i++)
        ids[i] = CZ_EINVAL;
    if (!slots || !ids)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    const bool direct = b->device == engine_device(e) && b->state.ptr;
    std::vector<SessionItem> items(count);
    for (uint32_t i = 0; i < count; i++) {
        const Slot *s = b->slot(slots[i]);
        if (!s || s->state != SLOT_CONNECTED) {
            items[i] = SessionItem{0, 0, 0, nullptr, 0, 0};
            continue;
        }
        items[i] = SessionItem{1, (uint8_t)(server ? 1 : 0), (uint64_t)b->state_size * (uint32_t)slots[i] + precom_off,
                               s->precom, next_nonce, s->peer_nonce};
    }
    return engine_add_sessions(e, where, count, items.data(), direct ? b->state.ptr : nullptr, ids);
}

// hs_release for a list, all or nothing: every slot must be in use and none named twice, else
// CZ_EINVAL with nothing released.  The device records are wiped by one k_scatter_wipe launch on the
// handshake's stream, before any later stage can hand a slot to another connection; the slots are
// freed in list order.
template <class Slot>
int hs_release_batch(HsBatch<Slot> *b, const char *where, uint32_t count, const int32_t *slots)
{
    if (!b)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    if (count == 0)
        return CZ_OK;
    if (!slots)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    for (uint32_t i = 0; i < count; i++) {
        const Slot *s = b->slot(slots[i]);
        if (!s || s->state == SLOT_FREE)
            return fail(CZ_EINVAL, "%s: slot %d is not in use", where, slots[i]);
    }
    {
        std::vector<int32_t> sorted(slots, slots + count);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end())
            return fail(CZ_EINVAL, "%s: slot %d is named twice", where, *dup);
    }
    hipError_t e;
    if ((e = hipSetDevice(b->device)) != hipSuccess || (e = b->h_rel.reserve(4ull * count)) != hipSuccess ||
        (e = b->d_rel.reserve(4ull * count)) != hipSuccess)
        return hip_fail(e, where);
    memcpy(b->h_rel.ptr, slots, 4ull * count);  // checked above: every id is in [0, max_pending)
    // (the synchronisation lets the next call reuse the pinned list)
    if ((e = hipMemcpyAsync(b->d_rel.ptr, b->h_rel.ptr, 4ull * count, hipMemcpyHostToDevice, b->stream)) != hipSuccess ||
        (e = czk_scatter_wipe(b->state.ptr, (const uint32_t *)b->d_rel.ptr, count, b->state_size, 0, b->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(b->stream)) != hipSuccess)
        return hip_fail(e, where);
    for (uint32_t i = 0; i < count; i++)
        b->free_slot(slots[i]);
    return CZ_OK;
}

template <class Slot>
int hs_peer_property(const HsBatch<Slot> *b, const char *where, int32_t slot, const char *name, const uint8_t **value,
                     uint32_t *len)
{
    if (!b || !name || !value || !len)
        return fail(CZ_EINVAL, "%s: null pointer", where);
    const Slot *s = b->slot(slot);
    if (s && s->state != SLOT_FREE)
        for (const auto &p : s->peer)
            if (p.first == name) {
                *value = p.second.data();
                *len = (uint32_t)p.second.size();
                return CZ_OK;
            }
    return fail(CZ_EINVAL, "%s: no property %s on slot %d", where, name, slot);
}

template <class Slot>
int hs_release(HsBatch<Slot> *b, const char *where, int32_t slot)
{
    Slot *s = b ? b->slot(slot) : nullptr;
    if (!s || s->state == SLOT_FREE)
        return fail(CZ_EINVAL, "%s: slot %d is not in use", where, slot);
    hipError_t e;
    if ((e = hipSetDevice(b->device)) != hipSuccess || (e = b->wipe_record(slot)) != hipSuccess)
        return hip_fail(e, where);
    b->free_slot(slot);
    return CZ_OK;
}

template <class Slot>
uint32_t hs_pending(const HsBatch<Slot> *b)
{
    return b ? b->max_pending - (uint32_t)b->free_slots.size() : 0;
}

// what one lane of a stage takes: key agreements (cza_job records), bytes of its input record, of its
// share of x and of its output record; a stage without key agreements has no jobs and no x
struct LaneShape {
    uint32_t jobs, in_rec, x_rec, out_rec;
};

// Where a reserved stage's buffers are.  A stage function takes a copy and indexes it with its own
// record sizes, so its per-lane loops read no state but their own locals.
struct StageBuffers {
    cza_job *jobs;          // pinned host, to fill before run(): the job descriptors
    uint8_t *recs;          //   and the input records
    uint8_t *out;           // pinned host, to read after run(): the output records
    const cza_job *d_jobs;  // the same on the device, for the job descriptors and the launches
    uint8_t *d_recs, *d_x, *d_out;
};

// One stage call over nj lanes.  reserve(), then fill the jobs and records of buffers() (every byte the
// kernels read: the staging is not cleared first), then run() with the stage's launches, then status()
// per lane.
template <class Slot>
class Stage {
public:
    // name: the entry point, for messages.  wipe_out: the wipe at the end of the chain covers the output
    // records too, as it must where they carry cnPrecom; without it the wipe stops before them (the
    // two stages that hand out slots: their output is only a command for the wire).  fresh: the
    // results whose slots this call handed out, or nullptr; they go back if it fails.
    Stage(HsBatch<Slot> &b, const char *name, uint32_t nj, LaneShape lane, bool wipe_out, cz_accept_result *fresh)
        : b_(b), name_(name), nj_(nj), fresh_(fresh), jobs_b_(up16((uint64_t)lane.jobs * nj * sizeof(cza_job))),
          in_b_(jobs_b_ + (uint64_t)lane.in_rec * nj), out_off_(in_b_ + (uint64_t)lane.x_rec * nj),
          out_b_((uint64_t)lane.out_rec * nj), wipe_b_(wipe_out ? out_off_ + out_b_ : out_off_)
    {
    }

    int reserve()
    {
        hipError_t e;
        if ((e = hipSetDevice(b_.device)) != hipSuccess || (e = b_.work.reserve(out_off_ + out_b_)) != hipSuccess ||
            (e = b_.h_in.reserve(in_b_)) != hipSuccess || (e = b_.h_out.reserve(out_b_)) != hipSuccess) {
            hand_back();
            return fail(CZ_EHIP, "%s: buffers: %s", name_, hipGetErrorString(e));
        }
        h_ = (uint8_t *)b_.h_in.ptr;
        d_ = (uint8_t *)b_.work.ptr;
        return CZ_OK;
    }

    StageBuffers buffers() const
    {
        return StageBuffers{(cza_job *)h_, h_ + jobs_b_, (uint8_t *)b_.h_out.ptr,
                            (const cza_job *)d_, d_ + jobs_b_, d_ + in_b_, d_ + out_off_};
    }
    uint64_t out_bytes() const { return out_b_; }

    // the records could not be filled (no randomness): nothing was enqueued
    int abandon(int rc)
    {
        secure_wipe(h_, in_b_);
        hand_back();
        return rc;
    }

    // The chain and its one synchronisation; launches(stream) enqueues the stage's kernels and returns
    // the first error.  On any failure the staging is wiped on both sides.
    template <class Launches>
    int run(Launches launches)
    {
        hipError_t e;
        if ((e = hipMemsetAsync(d_ + out_off_, 0xff, out_b_, b_.stream)) != hipSuccess ||
            (e = hipMemcpyAsync(d_, h_, in_b_, hipMemcpyHostToDevice, b_.stream)) != hipSuccess ||
            (e = launches(b_.stream)) != hipSuccess ||
            (e = hipMemcpyAsync(b_.h_out.ptr, d_ + out_off_, out_b_, hipMemcpyDeviceToHost, b_.stream)) != hipSuccess ||
            (e = hipMemsetAsync(d_, 0, wipe_b_, b_.stream)) != hipSuccess ||
            (e = hipStreamSynchronize(b_.stream)) != hipSuccess) {
            b_.wipe_staging(out_off_ + out_b_, in_b_, out_b_);
            hand_back();
            return hip_fail(e, name_);
        }
        return CZ_OK;
    }

    // The status word lane j left in its output record, one of those the stage's kernels write
    // (`known`).  A lane that left none of them did not run, a device failure the runtime did not
    // report: r.rc and the call's rc become CZ_EHIP and the stage sees CZA_ST_NOT_RUN.
    uint32_t status(uint32_t j, const uint8_t *status_word, cz_accept_result &r,
                    std::initializer_list<uint32_t> known = {CZA_ST_OK, CZA_ST_CRYPTO})
    {
        uint32_t st;
        memcpy(&st, status_word, 4);
        for (uint32_t k : known)
            if (st == k)
                return st;
        r.rc = CZ_EHIP;
        rc = fail(CZ_EHIP, "%s: lane %u left no status", name_, j);
        return CZA_ST_NOT_RUN;
    }

    int rc = CZ_OK;  // what the stage function returns once its lanes are walked

private:
    void hand_back()
    {
        if (fresh_)
            b_.give_back(fresh_, nj_);
    }

    HsBatch<Slot> &b_;
    const char *name_;
    uint32_t nj_;
    cz_accept_result *fresh_;
    uint64_t jobs_b_, in_b_, out_off_, out_b_, wipe_b_;
    uint8_t *h_ = nullptr, *d_ = nullptr;
};

}  // namespace czi
