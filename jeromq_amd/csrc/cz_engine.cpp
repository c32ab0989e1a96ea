// cz_engine.cpp -- batching engine: many CURVE connections, one device batch per flush.
//
// The reference encrypts one message at a time on each connection's IO thread:
//   outEvent  (StreamEngine.java:467-535) pulls Msgs, mechanism.encode()s each one
//             (CurveClientMechanism.java:126-163) and V2Encoder-frames it
//             (V2Encoder.java:31-55) into an OUT_BATCH_SIZE buffer for the socket;
//   inEvent   (StreamEngine.java:379-465) V2Decoder-parses the received bytes
//             (V2Decoder.java:37-105) and decodeAndPush (:1067-1098) mechanism.decode()s
//             each frame (CurveClientMechanism.java:165-224), tearing the connection down at
//             the first failure.
// Here the messages of ALL connections are queued in a pinned arena (the ZMQ_MSG_ALLOCATOR
// role, zmq/msg/MsgAllocator.java:5-8) and handled per flush with one device batch:
//   flush_out: descriptors with each connection's next nonces -> H2D -> segmented seal into
//              128-byte aligned body slots -> k_v2_copy packs every connection's frames, in send
//              order, behind their V2 headers into one contiguous wire stream per connection ->
//              D2H into pinned memory, ready for the socket write.
//   flush_in:  host V2 parse of each connection's received bytes (one header per frame; a
//              partial frame waits for more bytes) -> H2D of the whole frames -> k_v2_copy unpacks
//              bodies into aligned slots -> segmented open with the nonce floor chained frame to
//              frame inside each connection (desc.prev) -> D2H -> per-connection delivery up to the
//              first failing frame, whose status becomes the connection's error event.
//   flush_forward: Proxy.forward (zmq/Proxy.java:140-160) for connections routed 1:1 with cz_engine_forward:
//              the received bytes go over as they lie, are scanned and re-sealed in place for the destination
//              (cz_relay_streams' chain, header section 3j), and come back as the destination's wire stream,
//              cut at the first rejected frame.  No delivery, no plaintext in memory.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

#include "cz_internal.h"
#include "cz_routes.h"
#include "cz_session.h"

// pipeline depth of a large flush: groups of >= 8 MiB of wire bytes, at most this many.  At 1 GiB
// per flush, 16 against 8: out 39.0 -> 40.9, in 38.0 -> 40.0 GiB/s (shorter pipeline fill and
// drain); 24 and 32 drop flush_out to 28 / 20 GiB/s (profiles/r03/engine_groups_ab_s9/s10.log).
#ifndef CZ_ENGINE_GROUPS
#define CZ_ENGINE_GROUPS 16
#endif

using namespace czi;

namespace {

constexpr uint64_t SLOT_ALIGN = 128;  // body / payload slots: line-staged stores, whole-line loads

// (flush_in's segment length, flush_seg_blocks: cz_internal.h, shared with cz_plan_fanin_split)

uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// CZ_ENGINE_TRACE=1: per-phase wall times of each flush on stderr (profiling aid)
struct PhaseTimer {
    bool on;
    const char *what;
    std::chrono::steady_clock::time_point t0, last;
    char buf[512];
    int len = 0;
    explicit PhaseTimer(const char *w) : on(getenv("CZ_ENGINE_TRACE") != nullptr), what(w)
    {
        t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char *phase)
    {
        if (!on)
            return;
        auto now = std::chrono::steady_clock::now();
        len += snprintf(buf + len, sizeof(buf) - len, " %s=%.2fms", phase,
                        std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
    ~PhaseTimer()
    {
        if (on)
            fprintf(stderr, "[cz_engine] %s%s total=%.2fms\n", what, buf,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

struct Run {
    uint64_t off, len;
};

// A connection's receive buffer: a region of one of the engine's pinned receive blocks.
struct RxBuf {
    uint8_t *ptr = nullptr;
    uint64_t cap = 0;
    uint32_t blk = 0;
};

// Pinned receive blocks shared by every connection.  Regions are bump-allocated, so connections
// that receive together lie next to each other and flush_in moves a run of them with one DMA
// (each DMA costs a ~25 us gap on the SDMA queue, about the time of a 1 MiB copy).  A region that
// grows extends in place when it is the last one of its block; otherwise it moves and its old
// space goes to a first-fit free list.
struct RxPool {
    struct Block {
        uint8_t *base;
        uint64_t cap, used;
    };
    std::vector<Block> blocks;
    std::vector<RxBuf> free_list;
    uint64_t total = 0;

    ~RxPool()
    {
        for (Block &b : blocks)
            (void)hipHostFree(b.base);
    }
    // grow r to hold `want` bytes, keeping its first `used` bytes
    hipError_t grow(RxBuf &r, uint64_t used, uint64_t want)
    {
        if (want <= r.cap)
            return hipSuccess;
        const uint64_t cap = (std::max<uint64_t>({want, 2 * r.cap, 65536}) + 255) & ~255ull;
        if (r.ptr) {
            Block &b = blocks[r.blk];
            if (r.ptr + r.cap == b.base + b.used && b.used - r.cap + cap <= b.cap) {
                b.used += cap - r.cap;
                r.cap = cap;
                return hipSuccess;
            }
        }
        RxBuf n;
        size_t fi = 0;
        for (; fi < free_list.size() && free_list[fi].cap < cap; fi++) {
        }
        if (fi < free_list.size()) {
            n = free_list[fi];
            free_list.erase(free_list.begin() + (long)fi);
        } else {
            if (blocks.empty() || blocks.back().cap - blocks.back().used < cap) {
                // blocks grow with the pool: 1 MiB .. 256 MiB, or one region's size
                const uint64_t bcap = std::max<uint64_t>(cap, std::min<uint64_t>(256ull << 20,
                                                                                std::max<uint64_t>(1ull << 20, total)));
                void *p = nullptr;
                hipError_t e = hipHostMalloc(&p, bcap, hipHostMallocDefault);
                if (e != hipSuccess)
                    return e;
                blocks.push_back({(uint8_t *)p, bcap, 0});
                total += bcap;
            }
            Block &b = blocks.back();
            n = {b.base + b.used, cap, (uint32_t)(blocks.size() - 1)};
            b.used += cap;
        }
        if (used)
            memcpy(n.ptr, r.ptr, used);
        if (r.ptr)
            free_list.push_back(r);
        r = n;
        return hipSuccess;
    }
};

// Received bytes go to the device as they lie in the pinned receive blocks, one DMA per span: a run of
// connections in address order, merged while they share a receive block and the bytes between them (other
// connections' spare capacity) are at most MERGE_GAP -- copying those costs less than another DMA's gap.
struct Span {
    const uint8_t *src;
    uint64_t dev, len;
};

// Where the next connection's `rx_len` received bytes go in d_wire: into the last span of spans[first ...] when
// it merges, else a new span at `off`, the running device offset.  blk: the receive block of that last span.
uint64_t place_in_spans(std::vector<Span> &spans, size_t first, uint32_t &blk, uint64_t &off, const RxBuf &rx,
                        uint64_t rx_len)
{
    constexpr uint64_t MERGE_GAP = 1ull << 20;
    Span *last = spans.size() > first ? &spans.back() : nullptr;
    if (last && rx.blk == blk && rx.ptr <= last->src + last->len + MERGE_GAP) {
        const uint64_t at = last->dev + (uint64_t)(rx.ptr - last->src);
        const uint64_t end = (uint64_t)(rx.ptr + rx_len - last->src);
        off += end - last->len;
        last->len = end;
        return at;
    }
    const uint64_t at = off;
    spans.push_back({rx.ptr, off, rx_len});
    off += rx_len;
    blk = rx.blk;
    return at;
}

struct Conn {
    bool server = false;
    uint32_t tx_key = 0, rx_key = 0;  // subkey table indices
    uint64_t nonce = 0;               // cnNonce: next MESSAGE nonce to send
    uint64_t peer_nonce = 0;          // cnPeerNonce: last accepted peer nonce
    int error = 0;                    // CZ_EPROTO / CZ_EMSGSIZE once torn down
    int event = 0;                    // ZMTP protocol-error event of the failure
    RxBuf rx;                         // received bytes not yet parsed, pinned (DMA'd as they lie)
    uint64_t rx_len = 0;
    std::vector<Run> runs;            // wire stream of the last flush_out: pieces of h_wire, in send order
    std::vector<uint8_t> gathered;    // contiguous copy for cz_engine_wire_out when runs > 1
    std::vector<uint32_t> in_msgs;    // indices into Engine::in_msgs of the last flush_in
    uint64_t fwd_off = 0, fwd_len = 0;  // what the last flush_forward made of its received bytes: a piece of h_fwd
    bool removed = false;             // cz_engine_remove_conn: the id and its key slots await reuse
};

struct OutMsg {
    uint32_t conn;
    uint64_t arena_off;
    uint32_t len;
    uint32_t flags;
    uint32_t pub = 0;  // cz_engine_publish call this frame belongs to (0: cz_engine_send)
};

// A run of one publish's frames inside a flush group, one cz_fanout_run of the group's
// cz_seal_fanout_runs call: send-order frames [first, first + count) share payload, length and
// flags, and their body slots are contiguous at one stride.
struct FanRun {
    uint32_t first, count;
    bool split;  // the group's cz_seal_fanout_split call (subscriber x segment grid) instead
};

// The fan-out runs of pend[fa, fb): maximal runs of consecutive frames of one publish with at
// least `min_run` frames, or with at least one full wave of frames and a payload of at most
// `short_len` bytes (0: that rule off).  Of the other runs, those with at least one full wave of
// frames and a payload of at least `split_len` bytes (0: off) are split runs.  min_run 0: none.
void fanout_runs(const std::vector<OutMsg> &pend, uint32_t fa, uint32_t fb, uint32_t min_run, uint32_t short_len,
                 uint32_t split_len, std::vector<FanRun> &runs)
{
    runs.clear();
    if (min_run == 0)
        return;
    for (uint32_t i = fa; i < fb;) {
        uint32_t j = i + 1;
        if (pend[i].pub)
            while (j < fb && pend[j].pub == pend[i].pub)
                j++;
        if (pend[i].pub && (j - i >= min_run || (short_len && j - i >= 64u && pend[i].len <= short_len)))
            runs.push_back({i, j - i, false});
        else if (pend[i].pub && split_len && j - i >= 64u && pend[i].len >= split_len)
            runs.push_back({i, j - i, true});
        i = j;
    }
}

struct InMsg {
    uint64_t plain_off;
    uint32_t len;
    int flags;
};

struct Segs {
    std::vector<cz_segment> seg;
    std::vector<cz_combine> comb;
    uint32_t nseg = 0, ncomb = 0, npart = 0;
};

// destroys a flush's events on every return path
struct EvGuard {
    std::vector<hipEvent_t> &v;
    ~EvGuard()
    {
        for (hipEvent_t x : v)
            if (x)
                (void)hipEventDestroy(x);
    }
};

}  // namespace

struct cz_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    // flush pipelines: ps[0] carries every group's H2D in order; ps[1] waits for a group's copies
    // (event) and runs its kernels; ps[2] waits for those (event) and carries the group's D2H -- so
    // group g's D2H overlaps group g+1's H2D and kernels
    static constexpr int PIPE = 3;
    hipStream_t ps[PIPE] = {nullptr, nullptr, nullptr};
    std::vector<Conn> conns;
    std::vector<int> free_ids;  // removed connections, reused (with their subkey slots) by add_conn
    DevBuf subkeys;  // 32 B per (connection, direction)
    uint32_t nkeys = 0;
    // outbound
    HostBuf arena;
    uint64_t arena_cap = 0, arena_used = 0;
    std::vector<OutMsg> pend;
    HostBuf h_wire;
    uint64_t wire_total = 0;
    // inbound
    HostBuf h_plain;
    std::vector<InMsg> in_msgs;
    // device staging (grows, never shrinks)
    DevBuf d_in, d_body, d_wire, d_desc, d_seg, d_comb, d_work, d_items, d_status, d_nonces, d_plain, d_subs,
        d_fruns, d_fwaves,  // grouped fan-out: run and wave tables
        d_ftiles, d_fjoins, d_fwork;  // split fan-out: tile and join tables, partial records
    uint32_t pub_seq = 0;  // id of the last cz_engine_publish call (OutMsg::pub)
    uint64_t fanin_frames = 0;  // frames of the last flush_in that its cz_open_fanin_runs calls opened
    uint64_t fanin_split_frames = 0;  // ... and that its cz_open_fanin_split calls opened
    uint64_t scan_frames = 0;  // ... and that the scanned path opened (cz_tune "scan_in": the whole flush or nothing)
    // scanned flush: one cz_v2_stream per receiving connection, its cz_v2_stream_result, then the totals record
    DevBuf d_scan;
    HostBuf h_scan;
    // forward routes (cz_engine_forward): flush_forward re-seals a routed connection's received stream in place
    // for its destination; the wire bytes come back into h_fwd
    RouteTable routes;
    HostBuf h_fwd;
    uint64_t forward_frames = 0;  // frames the last flush_forward forwarded
    HostBuf h_status, h_nonces;
    HostBuf h_meta;  // pinned staging of descriptors / items / segment lists (async H2D)
    RxPool rxpool;   // every connection's receive buffer
    // bulk add / remove (engine_add_sessions, cz_engine_remove_conns): staged precoms and job records, or the
    // key indices to wipe; reused from call to call, wiped before each call returns
    DevBuf d_stage;
    HostBuf h_stage;

    // wait for everything issued on every stream (error paths of the flushes: the next recv /
    // flush may write or regrow the pinned buffers those copies still read or write)
    void drain()
    {
        if (stream)
            (void)hipStreamSynchronize(stream);
        for (hipStream_t q : ps)
            if (q)
                (void)hipStreamSynchronize(q);
    }

    ~cz_engine()
    {
        if (stream) {
            (void)hipSetDevice(device);
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
        for (hipStream_t &q : ps)
            if (q) {
                (void)hipStreamSynchronize(q);
                (void)hipStreamDestroy(q);
            }
        for (DevBuf *b : {&subkeys, &d_in, &d_body, &d_wire, &d_desc, &d_seg, &d_comb, &d_work, &d_items, &d_status,
                          &d_nonces, &d_plain, &d_subs, &d_fruns, &d_fwaves, &d_ftiles, &d_fjoins,
                          &d_fwork, &d_stage, &d_scan})
            b->release();
        for (HostBuf *b : {&arena, &h_wire, &h_plain, &h_status, &h_nonces, &h_meta, &h_stage, &h_scan, &h_fwd})
            b->release();
    }

    Conn *conn(int c)
    {
        if (c < 0 || (size_t)c >= conns.size() || conns[(size_t)c].removed) {
            fail(CZ_EINVAL, "cz_engine: unknown connection %d", c);
            return nullptr;
        }
        return &conns[(size_t)c];
    }

    // grow the device subkey table to hold `want` keys, keeping its contents
    hipError_t grow_keys(uint32_t want)
    {
        if ((uint64_t)want * 32 <= subkeys.cap)
            return hipSuccess;
        void *p = nullptr;
        const uint64_t bytes = std::max<uint64_t>(4096, (uint64_t)want * 64);
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess)
            return e;
        if (nkeys && (e = hipMemcpyAsync(p, subkeys.ptr, (uint64_t)nkeys * 32, hipMemcpyDeviceToDevice, stream)) !=
                         hipSuccess)
            return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess)
            return e;
        subkeys.release();
        subkeys.ptr = p;
        subkeys.cap = bytes;
        return hipSuccess;
    }

    // Outbound pipeline.  The wire output is in SEND order: message i's V2 frame (header + body)
    // sits at wpos[i], and each connection's stream is the list of its runs of consecutive frames
    // (one run when the caller queued a connection's messages together, as StreamEngine.outEvent
    // pulls one pipe at a time).  Send order lets the flush run in G groups of ~equal bytes:
    // ps[0] copies group g's arena range and metadata while ps[1] seals + packs group g-1 and
    // copies its wire bytes back, so H2D and D2H overlap instead of running back to back.
    int flush_out()
    {
        PhaseTimer pt("flush_out");
        for (Conn &c : conns) {
            c.runs.clear();
            c.gathered.clear();
        }
        wire_total = 0;
        const uint32_t n = (uint32_t)pend.size();
        if (n == 0) {
            arena_used = 0;  // buffers allocated but never sent are released too
            return CZ_OK;
        }
        // 1. send-order wire positions and each connection's runs
        std::vector<uint64_t> wpos(n + 1);
        uint64_t w = 0, longest = 0;
        for (uint32_t i = 0; i < n; i++) {
            const OutMsg &m = pend[i];
            Conn &c = conns[m.conn];
            const uint64_t body = (uint64_t)m.len + CZ_MESSAGE_OVERHEAD;
            longest = std::max<uint64_t>(longest, body);
            const uint64_t fb = cz_v2_header_size(body) + body;
            wpos[i] = w;
            if (!c.runs.empty() && c.runs.back().off + c.runs.back().len == w)
                c.runs.back().len += fb;
            else
                c.runs.push_back({w, fb});
            w += fb;
        }
        wpos[n] = w;
        wire_total = w;
        const uint32_t seg = batch_seg_blocks(w / 64, (longest + 63) / 64);
        // 2. groups of ~equal wire bytes: [fa, fb) in send order, body slots contiguous per group;
        //    per group the arena prefix it needs, its body-slot base and its segment / combine
        //    counts (plan_counts) -- enough to size every buffer and start the arena copy before
        //    any descriptor exists
        struct Group {
            uint32_t fa, fb;
            uint64_t arena_hi;  // the arena prefix [0, arena_hi) holds every payload of groups <= this one
            uint64_t slot0;     // first body slot
        };
        std::vector<Group> groups;
        {
            const uint64_t G = std::min<uint64_t>(CZ_ENGINE_GROUPS, std::max<uint64_t>(1, w / (8ull << 20)));
            uint32_t fa = 0;
            for (uint32_t i = 0; i < n; i++)
                if (i + 1 == n || wpos[i + 1] * G >= w * (groups.size() + 1)) {
                    groups.push_back({fa, i + 1, 0, 0});
                    fa = i + 1;
                }
        }
        // publishes: inside a group, a run of one publish's frames has contiguous body slots of
        // one stride (slots follow send order) and leaves the segment plan for the group's one
        // cz_seal_fanout_runs call; a publish split by a group edge is two runs.  fan[i]: frame i
        // is in such a run.  roff / fwoff: the groups' ranges in the run and wave tables.  The split
        // runs of a group (cz_tune "fanout_split") are its one cz_seal_fanout_split call at the
        // flush's segment length: toff / joff / pwoff, its ranges of tiles, joins and partial records.
        std::vector<std::vector<FanRun>> fruns(groups.size());
        std::vector<uint8_t> fan(n, 0);
        std::vector<uint64_t> roff(groups.size() + 1, 0), fwoff(groups.size() + 1, 0), toff(groups.size() + 1, 0),
            joff(groups.size() + 1, 0), pwoff(groups.size() + 1, 0);
        const uint32_t fan_min = fanout_min(), fan_short = fanout_short(), fan_split = fanout_split();
        for (size_t gi = 0; gi < groups.size(); gi++) {
            fanout_runs(pend, groups[gi].fa, groups[gi].fb, fan_min, fan_short, fan_split, fruns[gi]);
            roff[gi + 1] = roff[gi] + fruns[gi].size();
            fwoff[gi + 1] = fwoff[gi];
            std::vector<cz_fanout_run> split;  // (length and count are all the counts need)
            for (const FanRun &r : fruns[gi]) {
                std::fill(fan.begin() + r.first, fan.begin() + r.first + r.count, (uint8_t)1);
                if (r.split)
                    split.push_back({0, 0, 0, pend[r.first].len, 0, 0, r.count});
                else
                    fwoff[gi + 1] += ((uint64_t)r.count + 63) / 64;
            }
            const FanoutSplitCounts sc = fanout_split_counts(split.data(), (uint32_t)split.size(), seg);
            if (sc.ntiles > 0xffffffffull || sc.npart > 0xffffffffull)
                return fail(CZ_EINVAL, "cz_engine: more than 2^32 - 1 fan-out tiles in a flush group");
            toff[gi + 1] = toff[gi] + sc.ntiles;
            joff[gi + 1] = joff[gi] + sc.njoins;
            pwoff[gi + 1] = pwoff[gi] + sc.npart;
        }
        const uint64_t nfrun = roff[groups.size()], nfwave = fwoff[groups.size()], nftile = toff[groups.size()],
                       nfjoin = joff[groups.size()], nfpart = pwoff[groups.size()];
        const bool any_fan = nfrun != 0;
        std::vector<uint64_t> soff(groups.size() + 1, 0), coff(groups.size() + 1, 0), woff(groups.size() + 1, 0);
        uint64_t slot = 0, hi = 0;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            Group &g = groups[gi];
            g.slot0 = slot;
            uint64_t ns = 0, nc = 0, np = 0;
            for (uint32_t i = g.fa; i < g.fb; i++) {
                const OutMsg &m = pend[i];
                slot += round_up((uint64_t)m.len + CZ_MESSAGE_OVERHEAD, SLOT_ALIGN);
                hi = std::max<uint64_t>(hi, m.arena_off + m.len);
                if (!fan[i])
                    plan_counts(m.len, 0, seg, ns, nc, np);
            }
            g.arena_hi = hi;
            soff[gi + 1] = soff[gi] + ns;
            coff[gi + 1] = coff[gi] + nc;
            woff[gi + 1] = woff[gi] + np;
        }
        const uint64_t nseg = soff[groups.size()], ncomb = coff[groups.size()], npart = woff[groups.size()];
        const uint64_t m_items = 0, m_desc = (uint64_t)n * sizeof(cz_v2_item),
                       m_seg = m_desc + (uint64_t)n * sizeof(cz_frame_desc), m_comb = m_seg + nseg * sizeof(cz_segment),
                       m_subs = m_comb + ncomb * sizeof(cz_combine),
                       m_fruns = m_subs + (any_fan ? (uint64_t)n * sizeof(cz_fanout_sub) : 0),
                       m_fwaves = m_fruns + nfrun * sizeof(cz_fanout_run),
                       m_ftiles = m_fwaves + nfwave * sizeof(cz_fanout_wave),
                       m_fjoins = m_ftiles + nftile * sizeof(cz_fanout_tile),
                       m_end = m_fjoins + nfjoin * sizeof(cz_fanout_join);
        hipError_t e;
        if ((e = d_in.reserve(std::max<uint64_t>(arena_used, 16))) != hipSuccess ||
            (e = d_body.reserve(slot)) != hipSuccess || (e = d_wire.reserve(wire_total)) != hipSuccess ||
            (e = d_items.reserve((uint64_t)n * sizeof(cz_v2_item))) != hipSuccess ||
            (e = d_desc.reserve((uint64_t)n * sizeof(cz_frame_desc))) != hipSuccess ||
            (e = d_seg.reserve(std::max<uint64_t>(nseg, 1) * sizeof(cz_segment))) != hipSuccess ||
            (e = d_comb.reserve(std::max<uint64_t>(ncomb, 1) * sizeof(cz_combine))) != hipSuccess ||
            (e = d_work.reserve(std::max<uint64_t>(npart, 1) * 64)) != hipSuccess ||
            (any_fan && ((e = d_subs.reserve((uint64_t)n * sizeof(cz_fanout_sub))) != hipSuccess ||
                         (e = d_fruns.reserve(nfrun * sizeof(cz_fanout_run))) != hipSuccess ||
                         (e = d_fwaves.reserve(nfwave * sizeof(cz_fanout_wave))) != hipSuccess ||
                         (e = d_ftiles.reserve(nftile * sizeof(cz_fanout_tile))) != hipSuccess ||
                         (e = d_fjoins.reserve(nfjoin * sizeof(cz_fanout_join))) != hipSuccess ||
                         (e = d_fwork.reserve(nfpart * 64)) != hipSuccess)) ||
            (e = h_wire.reserve(wire_total)) != hipSuccess || (e = h_meta.reserve(m_end)) != hipSuccess)
            return hip_fail(e, "cz_engine: alloc");
        // descriptors and items are built straight into pinned staging (pageable sources would
        // make each H2D synchronous), one group at a time while the copies issued before run
        uint8_t *hm = (uint8_t *)h_meta.ptr;
        cz_v2_item *h_items = (cz_v2_item *)(hm + m_items);
        cz_frame_desc *h_desc = (cz_frame_desc *)(hm + m_desc);
        cz_fanout_sub *h_subs = (cz_fanout_sub *)(hm + m_subs);  // by send index, fan-out frames only
        cz_fanout_run *h_fruns = (cz_fanout_run *)(hm + m_fruns);
        cz_fanout_wave *h_fwaves = (cz_fanout_wave *)(hm + m_fwaves);
        cz_fanout_tile *h_ftiles = (cz_fanout_tile *)(hm + m_ftiles);
        cz_fanout_join *h_fjoins = (cz_fanout_join *)(hm + m_fjoins);
        pt.mark("plan");
        std::vector<hipEvent_t> ev(groups.size(), nullptr), evk(groups.size(), nullptr);
        EvGuard evguard{ev}, evkguard{evk};
        for (size_t gi = 0; gi < groups.size(); gi++)
            if ((e = hipEventCreateWithFlags(&ev[gi], hipEventDisableTiming)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&evk[gi], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "hipEventCreate");
        // one group: no overlap to gain, so one stream and no cross-stream events (each costs
        // tens of us, the bulk of a small flush's latency)
        hipStream_t qh = ps[0], qk = ps[1], qo = ps[2];
        if (groups.size() == 1)
            qh = qo = qk;
        uint64_t copied = 0;
        // the arena bytes not copied yet up to group g's last payload
        auto copy_arena = [&](size_t gi) -> hipError_t {
            if (gi >= groups.size() || groups[gi].arena_hi <= copied)
                return hipSuccess;
            hipError_t r = hipMemcpyAsync((uint8_t *)d_in.ptr + copied, (const uint8_t *)arena.ptr + copied,
                                          groups[gi].arena_hi - copied, hipMemcpyHostToDevice, qh);
            copied = groups[gi].arena_hi;
            return r;
        };
        if ((e = copy_arena(0)) != hipSuccess)
            return hip_fail(e, "cz_engine: H2D");
        Segs sg;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const Group &g = groups[gi];
            const uint32_t gn = g.fb - g.fa;
            uint64_t bs = g.slot0;
            // nonces in send order; the group's descriptors (segment-plan frames only) are packed
            // at the front of its range -- cz_v2_item carries each frame's slot and wire position
            uint32_t gd = 0;
            for (uint32_t i = g.fa; i < g.fb; i++) {
                const OutMsg &m = pend[i];
                Conn &c = conns[m.conn];
                const uint64_t body = (uint64_t)m.len + CZ_MESSAGE_OVERHEAD;
                if (fan[i])
                    h_subs[i] = {c.nonce++, c.tx_key, 0u};
                else
                    h_desc[g.fa + gd++] = {m.arena_off, bs, m.len, c.tx_key, c.nonce++, m.flags & 0xffu, -1};
                h_items[i] = {bs, wpos[i], (uint32_t)body, (uint32_t)CZ_V2_ITEM_HEADER};
                bs += round_up(body, SLOT_ALIGN);
            }
            const std::vector<FanRun> &fr = fruns[gi];
            // one copy for the group's subscriber records: first run's start to last run's end
            const uint32_t sub_a = fr.empty() ? 0u : fr.front().first,
                           sub_b = fr.empty() ? 0u : fr.back().first + fr.back().count;
            // the group's run table (a run's first_sub is its send index): the gfr grouped runs and
            // their wave table, then the gsr split runs with their tile and join tables
            const uint32_t gsr = (uint32_t)std::count_if(fr.begin(), fr.end(), [](const FanRun &r) { return r.split; });
            const uint32_t gfr = (uint32_t)fr.size() - gsr, gfw = (uint32_t)(fwoff[gi + 1] - fwoff[gi]);
            const uint32_t gst = (uint32_t)(toff[gi + 1] - toff[gi]), gsj = (uint32_t)(joff[gi + 1] - joff[gi]);
            cz_fanout_run *hr = h_fruns + roff[gi];
            uint32_t fclass[3] = {0, 0, 0}, fregion = 0, sclass[2] = {0, 0};
            uint32_t kf = 0, ks = gfr;
            for (const FanRun &r : fr) {
                const OutMsg &m = pend[r.first];
                hr[r.split ? ks++ : kf++] = {m.arena_off, h_items[r.first].src_off,
                                             round_up((uint64_t)m.len + CZ_MESSAGE_OVERHEAD, SLOT_ALIGN), m.len,
                                             m.flags & 0xffu, r.first, r.count};
            }
            if (gfr)
                fregion = plan_fanout(hr, gfr, d_in.ptr, d_body.ptr, h_fwaves + fwoff[gi], fclass);
            if (gsr)
                plan_fanout_split(hr + gfr, gsr, d_in.ptr, seg, h_ftiles + toff[gi], sclass, h_fjoins + joff[gi]);
            if (sclass[0] + sclass[1] != gst)
                return fail(CZ_EINVAL, "cz_engine: fan-out tile plan disagrees with its count");
            const cz_fanout_run *dfr = (const cz_fanout_run *)d_fruns.ptr + roff[gi];
            const cz_fanout_wave *dfw = (const cz_fanout_wave *)d_fwaves.ptr + fwoff[gi];
            const cz_fanout_tile *dft = (const cz_fanout_tile *)d_ftiles.ptr + toff[gi];
            const cz_fanout_join *dfj = (const cz_fanout_join *)d_fjoins.ptr + joff[gi];
            plan_segments(h_desc + g.fa, gd, 0, seg, sg.seg, sg.comb, sg.npart);
            const uint32_t gseg = (uint32_t)sg.seg.size(), gcomb = (uint32_t)sg.comb.size();
            if (gseg != soff[gi + 1] - soff[gi] || gcomb != coff[gi + 1] - coff[gi] || sg.npart != woff[gi + 1] - woff[gi])
                return fail(CZ_EINVAL, "cz_engine: segment plan disagrees with its count");
            memcpy(hm + m_seg + soff[gi] * sizeof(cz_segment), sg.seg.data(), (uint64_t)gseg * sizeof(cz_segment));
            memcpy(hm + m_comb + coff[gi] * sizeof(cz_combine), sg.comb.data(), (uint64_t)gcomb * sizeof(cz_combine));
            cz_frame_desc *dd = (cz_frame_desc *)d_desc.ptr + g.fa;
            cz_segment *dsg = (cz_segment *)d_seg.ptr + soff[gi];
            cz_combine *dcb = (cz_combine *)d_comb.ptr + coff[gi];
            // (a) copy stream: the group's metadata, then the next group's arena bytes (copied while
            //     the host builds that group)
            if ((e = hipMemcpyAsync((cz_v2_item *)d_items.ptr + g.fa, h_items + g.fa, (uint64_t)gn * sizeof(cz_v2_item),
                                    hipMemcpyHostToDevice, qh)) != hipSuccess ||
                (gd && (e = hipMemcpyAsync(dd, h_desc + g.fa, (uint64_t)gd * sizeof(cz_frame_desc), hipMemcpyHostToDevice,
                                           qh)) != hipSuccess) ||
                (sub_b > sub_a && (e = hipMemcpyAsync((cz_fanout_sub *)d_subs.ptr + sub_a, h_subs + sub_a,
                                                      (uint64_t)(sub_b - sub_a) * sizeof(cz_fanout_sub),
                                                      hipMemcpyHostToDevice, qh)) != hipSuccess) ||
                (gfr + gsr && (e = hipMemcpyAsync((void *)dfr, hr, (uint64_t)(gfr + gsr) * sizeof(cz_fanout_run),
                                                  hipMemcpyHostToDevice, qh)) != hipSuccess) ||
                (gfr && (e = hipMemcpyAsync((void *)dfw, h_fwaves + fwoff[gi], (uint64_t)gfw * sizeof(cz_fanout_wave),
                                            hipMemcpyHostToDevice, qh)) != hipSuccess) ||
                (gst && (e = hipMemcpyAsync((void *)dft, h_ftiles + toff[gi], (uint64_t)gst * sizeof(cz_fanout_tile),
                                            hipMemcpyHostToDevice, qh)) != hipSuccess) ||
                (gsj && (e = hipMemcpyAsync((void *)dfj, h_fjoins + joff[gi], (uint64_t)gsj * sizeof(cz_fanout_join),
                                            hipMemcpyHostToDevice, qh)) != hipSuccess) ||
                (gseg &&(e = hipMemcpyAsync(dsg, (const cz_segment *)(hm + m_seg) + soff[gi],
                                             (uint64_t)gseg * sizeof(cz_segment), hipMemcpyHostToDevice, qh)) !=
                             hipSuccess) ||
                (gcomb && (e = hipMemcpyAsync(dcb, (const cz_combine *)(hm + m_comb) + coff[gi],
                                              (uint64_t)gcomb * sizeof(cz_combine), hipMemcpyHostToDevice, qh)) !=
                              hipSuccess) ||
                (qh != qk && (e = hipEventRecord(ev[gi], qh)) != hipSuccess) ||
                (e = copy_arena(gi + 1)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out H2D");
            // (b) compute stream: seal into body slots, pack behind V2 headers at the send-order
            //     wire positions; (c) D2H stream: the group's wire bytes back
            if (qh != qk && (e = hipStreamWaitEvent(qk, ev[gi], 0)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out");
            if (gfr && (e = czk_seal_fanout_runs(dfr, dfw, fclass, fregion, d_in.ptr, (const cz_fanout_sub *)d_subs.ptr,
                                                 subkeys.ptr, d_body.ptr, qk)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out fan-out");
            if (gsr && (e = czk_seal_fanout_split(dfr + gfr, dft, sclass, dfj, gsj, d_in.ptr, (const cz_fanout_sub *)d_subs.ptr,
                                                  subkeys.ptr, d_body.ptr, (uint8_t *)d_fwork.ptr + 64 * pwoff[gi],
                                                  qk)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out split fan-out");
            if ((gseg &&(e = czk_seal_segments(dd, dsg, gseg, dcb, gcomb, d_in.ptr, d_body.ptr, subkeys.ptr,
                                                (uint8_t *)d_work.ptr + 64 * woff[gi], qk)) != hipSuccess) ||
                (e = czk_v2_copy((const cz_v2_item *)d_items.ptr + g.fa, gn, d_body.ptr, d_wire.ptr, qk)) !=
                    hipSuccess ||
                (qo != qk && ((e = hipEventRecord(evk[gi], qk)) != hipSuccess ||
                              (e = hipStreamWaitEvent(qo, evk[gi], 0)) != hipSuccess)) ||
                (e = hipMemcpyAsync((uint8_t *)h_wire.ptr + wpos[g.fa], (uint8_t *)d_wire.ptr + wpos[g.fa],
                                    wpos[g.fb] - wpos[g.fa], hipMemcpyDeviceToHost, qo)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out");
        }
        for (hipStream_t q : ps)
            if ((e = hipStreamSynchronize(q)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_out");
        pt.mark("h2d+kernels+d2h");
        pend.clear();
        arena_used = 0;
        return CZ_OK;
    }

    static int event_for(uint32_t status, bool server)
    {
        switch (status) {
        case CZ_STATUS_COMMAND: return CZ_ZMTP_UNEXPECTED_COMMAND;
        case CZ_STATUS_MALFORMED: return CZ_ZMTP_MALFORMED_COMMAND_MESSAGE;
        case CZ_STATUS_SEQUENCE: return server ? CZ_ZMTP_INVALID_SEQUENCE : CZ_ZMTP_CRYPTOGRAPHIC;
        default: return CZ_ZMTP_CRYPTOGRAPHIC;
        }
    }

    int flush_in()
    {
        PhaseTimer pt("flush_in");
        in_msgs.clear();
        fanin_frames = 0;
        fanin_split_frames = 0;
        scan_frames = 0;
        for (Conn &c : conns)
            c.in_msgs.clear();
        // 0. the live connections, in groups of ~equal received bytes
        struct Parsed {
            uint32_t conn;
            uint32_t first, count;  // range in frames
            uint64_t rx_off;        // where the connection's received bytes start in d_wire
            uint64_t consumed;      // whole frames
            int perr;               // framing error after the parsed frames
        };
        std::vector<Parsed> parsed;
        uint64_t rx_total = 0;
        for (size_t ci = 0; ci < conns.size(); ci++) {
            Conn &c = conns[ci];
            if (c.error || c.rx_len == 0 || routes.dest((int)ci) != -1)  // (a routed one waits for flush_forward)
                continue;
            parsed.push_back({(uint32_t)ci, 0u, 0u, 0u, 0u, 0});
            rx_total += c.rx_len;
        }
        // The scanned flush (cz_tune "scan_in" = n > 0): at least one full wave of connections, none holding more
        // than n bytes -- which bounds a lane's header walk and the longest frame one lane may have to open.
        const uint32_t scan_n = scan_in();
        bool scanned = scan_n && parsed.size() >= 64;
        for (size_t q = 0; scanned && q < parsed.size(); q++)
            scanned = conns[parsed[q].conn].rx_len <= scan_n;
        const uint32_t seg = flush_seg_blocks(rx_total / 64);
        struct Group {
            size_t pa, pb;        // parsed[pa, pb)
            uint32_t fa, fb;      // frames[fa, fb)
            uint64_t pl0, pl1;    // plaintext slot range
        };
        std::vector<Group> groups;
        {
            const int G = rx_total >= (64ull << 20) && !scanned ? CZ_ENGINE_GROUPS : 1;  // (scanned: always one)
            size_t pa = 0;
            uint64_t acc = 0;
            for (size_t q = 0; q < parsed.size(); q++) {
                acc += conns[parsed[q].conn].rx_len;
                if (q + 1 == parsed.size() || acc * G >= rx_total * (groups.size() + 1)) {
                    groups.push_back({pa, q + 1, 0, 0, 0, 0});
                    pa = q + 1;
                }
            }
        }
        hipError_t e;
        std::vector<hipEvent_t> evm(groups.size(), nullptr), evk(groups.size(), nullptr);
        EvGuard evmguard{evm}, evkguard{evk};
        for (size_t gi = 0; gi < groups.size(); gi++)
            if ((e = hipEventCreateWithFlags(&evm[gi], hipEventDisableTiming)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&evk[gi], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "hipEventCreate");
        // ps[0]: received bytes H2D straight from the pinned receive blocks, one DMA per run of
        // connections that lie next to each other there (RxPool), every group issued before any
        // parsing so the copies run while the host parses and plans; `stream`: metadata H2D;
        // ps[1]: unpack + open; ps[2]: D2H.  (A gather kernel reading the receive buffers over PCIe
        // instead of DMAs measured slower, and so did spreading the DMAs over two streams, gathering
        // each group into one pinned slab on 8 host threads (the memcpy is slower than the gaps it
        // removes) and hipMemcpyBatchAsync of the per-connection copies (the same gaps).)
        hipStream_t qh = ps[0], qk = ps[1], qo = ps[2], qm = stream;
        if (groups.size() <= 1)  // as flush_out: one group, one stream
            qh = qo = qm = qk;
        std::vector<hipEvent_t> ev(groups.size(), nullptr);
        EvGuard evguard{ev};
        for (size_t gi = 0; gi < groups.size(); gi++)
            if ((e = hipEventCreateWithFlags(&ev[gi], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "hipEventCreate");
        // spans (place_in_spans): each group's connections in address order
        std::vector<Span> spans;
        std::vector<size_t> span_end(groups.size());
        {
            uint64_t off = 0;
            std::vector<size_t> order;
            for (size_t gi = 0; gi < groups.size(); gi++) {
                order.clear();
                for (size_t pi = groups[gi].pa; pi < groups[gi].pb; pi++)
                    order.push_back(pi);
                std::sort(order.begin(), order.end(),
                          [&](size_t x, size_t y) { return conns[parsed[x].conn].rx.ptr < conns[parsed[y].conn].rx.ptr; });
                uint32_t blk = 0;
                for (size_t pi : order) {
                    const Conn &c = conns[parsed[pi].conn];
                    parsed[pi].rx_off = place_in_spans(spans, gi ? span_end[gi - 1] : 0, blk, off, c.rx, c.rx_len);
                }
                span_end[gi] = spans.size();
            }
            // (scanned: the open reads a frame's replay floor at bytes [8, 16) of the frame before it where they lie)
            if (off && (e = d_wire.reserve(off + (scanned ? 16 : 0))) != hipSuccess)
                return hip_fail(e, "cz_engine: alloc");
        }
        for (size_t gi = 0, si = 0; gi < groups.size(); gi++) {
            for (; si < span_end[gi]; si++)
                if ((e = hipMemcpyAsync((uint8_t *)d_wire.ptr + spans[si].dev, spans[si].src, spans[si].len,
                                        hipMemcpyHostToDevice, qh)) != hipSuccess)
                    return hip_fail(e, "cz_engine: H2D");
            if (qh != qk && (e = hipEventRecord(ev[gi], qh)) != hipSuccess)
                return hip_fail(e, "cz_engine: H2D");
        }
        pt.mark("h2d-issue");
        // 1. per group, on its own host thread: parse each connection's whole frames (V2Decoder; a
        //    partial frame waits for more bytes) and count the group's frames, body / plaintext slot
        //    bytes and segments (plan_counts) -- enough to place every group's arrays.
        struct GroupWork {
            std::vector<cz_v2_frame> frames;
            Segs sg;
            uint64_t bslot = 0, pslot = 0;   // slot bytes of the group
            uint64_t nseg = 0, ncomb = 0, npart = 0;
            uint64_t b0 = 0, soff = 0, coff = 0, woff = 0;  // where its arrays start
            bool bad_plan = false;
            // fan-in: maximal runs of consecutive frames of one body size (group-relative first frame),
            // at least one full wave of them with a payload of at most cz_tune("fanin_short") bytes.
            // Their body and plaintext slots are contiguous at one stride each, so a run is one
            // cz_fanin_run of the group's cz_open_fanin_runs call and leaves the segment plan; it may
            // span connection edges.  routed[i]: frame i is in such a run.
            std::vector<std::pair<uint32_t, uint32_t>> runs;  // (first, count)
            std::vector<uint8_t> routed;
            uint64_t nfwave = 0, nrouted = 0;
            // split fan-in: the other such runs whose payload is at least cz_tune("fanin_split") bytes are
            // the group's cz_open_fanin_split call at the flush's own segment length: they extend the run
            // table, and their tiles, joins and partial records are counted here, before any descriptor
            // exists (fanin_split_counts, as plan_counts for the segment plan)
            std::vector<std::pair<uint32_t, uint32_t>> sruns;  // (first, count)
            uint64_t stiles = 0, sjoins = 0, spart = 0, nsrouted = 0;
            // its fan-in block in the metadata staging and in d_subs: records by group-relative frame index,
            // then the run table (fan-in runs, then split runs), the wave table, the tile table and the
            // join table -- one upload
            uint64_t foff = 0, fbytes = 0;
            uint32_t fclass[3] = {0, 0, 0}, fregion = 0, sclass[2] = {0, 0};
        };
        std::vector<GroupWork> gw(groups.size());
        const uint32_t fin_short = fanin_short(), fin_split = fanin_split();
        auto parse = [&](size_t gi) {
            GroupWork &w = gw[gi];
            const Group &g = groups[gi];
            constexpr uint32_t CH = 4096;  // parse in chunks of CH frames
            for (size_t q = g.pa; q < g.pb; q++) {
                Parsed &p = parsed[q];
                const Conn &c = conns[p.conn];
                const size_t base = w.frames.size();
                uint64_t consumed = 0;
                int prc = CZ_OK;
                for (;;) {
                    const size_t at = w.frames.size();
                    w.frames.resize(at + CH);
                    uint32_t nf = 0;
                    uint64_t used = 0;
                    prc = cz_v2_parse((const uint8_t *)c.rx.ptr + consumed, c.rx_len - consumed, -1,
                                      w.frames.data() + at, CH, &nf, &used);
                    w.frames.resize(at + nf);
                    for (uint32_t k = 0; k < nf; k++)
                        w.frames[at + k].body_off += consumed;
                    consumed += used;
                    if (prc != CZ_OK || nf < CH)
                        break;
                }
                p.first = (uint32_t)base;  // group-relative until step 2
                p.count = (uint32_t)(w.frames.size() - base);
                p.consumed = consumed;
                p.perr = prc == CZ_OK ? 0 : prc;
            }
            const uint32_t gn = (uint32_t)w.frames.size();
            for (uint32_t i = 0; (fin_short || fin_split) && i < gn;) {
                uint32_t j = i + 1;
                while (j < gn && w.frames[j].size == w.frames[i].size)
                    j++;
                const bool full = j - i >= 64u && w.frames[i].size >= CZ_MESSAGE_OVERHEAD;
                const uint32_t plen = full ? w.frames[i].size - CZ_MESSAGE_OVERHEAD : 0u;
                const bool by_short = full && fin_short && plen <= fin_short;  // (keeps precedence)
                const bool by_split = full && !by_short && fin_split && plen >= fin_split;
                if (by_short || by_split) {
                    if (w.routed.empty())
                        w.routed.assign(gn, 0);
                    std::fill(w.routed.begin() + i, w.routed.begin() + j, (uint8_t)1);
                }
                if (by_short) {
                    w.runs.push_back({i, j - i});
                    w.nfwave += ((uint64_t)(j - i) + 63) / 64;
                    w.nrouted += j - i;
                }
                if (by_split) {
                    const cz_fanin_run one{0, 0, 0, 0, w.frames[i].size, 0u, j - i, 0u};
                    const FanoutSplitCounts sc = fanin_split_counts(&one, 1, seg);
                    w.sruns.push_back({i, j - i});
                    w.stiles += sc.ntiles;
                    w.sjoins += sc.njoins;
                    w.spart += sc.npart;
                    w.nsrouted += j - i;
                }
                i = j;
            }
            if (w.stiles > 0xffffffffull || w.spart > 0xffffffffull)
                w.bad_plan = true;
            for (uint32_t i = 0; i < gn; i++) {
                const cz_v2_frame &f = w.frames[i];
                const uint64_t plen = f.size > CZ_MESSAGE_OVERHEAD ? f.size - CZ_MESSAGE_OVERHEAD : 0;
                w.bslot += round_up(std::max<uint64_t>(f.size, 1), SLOT_ALIGN);
                w.pslot += round_up(std::max<uint64_t>(plen, 1), SLOT_ALIGN);
                if (w.routed.empty() || !w.routed[i])  // (the routed frames get no segments)
                    plan_counts(f.size, 1, seg, w.nseg, w.ncomb, w.npart);
            }
        };
        if (scanned) {
            // 1s. The scanned flush, on the one stream of a one-group flush: a 32-byte record per connection
            //     goes up, the device walks every connection's headers (one lane each) and places the streams,
            //     and the totals come back with the per-stream results -- the one extra synchronisation, which
            //     sizes the buffers.  Then the emitted descriptors open every frame from d_wire itself.  What
            //     comes back fills exactly what the host parse and build fill below: Parsed, the descriptors
            //     (for out_off / len), statuses and nonces.
            const uint32_t ns = (uint32_t)parsed.size();
            const uint64_t o_res = (uint64_t)ns * sizeof(cz_v2_stream),
                           o_tot = o_res + (uint64_t)ns * sizeof(cz_v2_stream_result);
            if ((e = h_scan.reserve(o_tot + sizeof(cz_v2_totals))) != hipSuccess ||
                (e = d_scan.reserve(o_tot + sizeof(cz_v2_totals))) != hipSuccess)
                return hip_fail(e, "cz_engine: alloc");
            cz_v2_stream *h_streams = (cz_v2_stream *)h_scan.ptr;
            for (uint32_t q = 0; q < ns; q++) {
                const Conn &c = conns[parsed[q].conn];
                h_streams[q] = {parsed[q].rx_off, c.rx_len, c.peer_nonce, c.rx_key, 0u};
            }
            const cz_v2_stream *d_streams = (const cz_v2_stream *)d_scan.ptr;
            cz_v2_stream_result *d_res = (cz_v2_stream_result *)((uint8_t *)d_scan.ptr + o_res);
            const cz_v2_stream_result *h_res = (const cz_v2_stream_result *)((const uint8_t *)h_scan.ptr + o_res);
            const cz_v2_totals *h_tot = (const cz_v2_totals *)((const uint8_t *)h_scan.ptr + o_tot);
            if ((e = hipMemcpyAsync(d_scan.ptr, h_streams, o_res, hipMemcpyHostToDevice, qk)) != hipSuccess ||
                (e = czk_v2_scan(d_streams, ns, d_wire.ptr, -1, (uint32_t)SLOT_ALIGN, d_res,
                                 (cz_v2_totals *)((uint8_t *)d_scan.ptr + o_tot), qk)) != hipSuccess ||
                (e = hipMemcpyAsync((uint8_t *)h_scan.ptr + o_res, d_res, o_tot + sizeof(cz_v2_totals) - o_res,
                                    hipMemcpyDeviceToHost, qk)) != hipSuccess ||
                (e = hipStreamSynchronize(qk)) != hipSuccess) {
                drain();
                return hip_fail(e, "cz_engine: flush_in scan");
            }
            pt.mark("scan");
            if (h_tot->nframes > 0x7fffffffull)
                return fail(CZ_EINVAL, "cz_engine: more than 2^31 - 1 received frames in one flush");
            const uint32_t sn = (uint32_t)h_tot->nframes;
            const uint64_t spl = h_tot->slot_bytes;
            if (sn) {
                if ((e = d_plain.reserve(spl)) != hipSuccess || (e = d_status.reserve((uint64_t)sn * 2)) != hipSuccess ||
                    (e = d_nonces.reserve((uint64_t)sn * 8)) != hipSuccess ||
                    (e = d_desc.reserve((uint64_t)sn * sizeof(cz_frame_desc))) != hipSuccess ||
                    (e = h_plain.reserve(spl)) != hipSuccess || (e = h_status.reserve((uint64_t)sn * 2)) != hipSuccess ||
                    (e = h_nonces.reserve((uint64_t)sn * 8)) != hipSuccess ||
                    (e = h_meta.reserve((uint64_t)sn * sizeof(cz_frame_desc))) != hipSuccess)
                    return hip_fail(e, "cz_engine: alloc");
                // (the descriptors land at the start of the metadata staging, where the delivery step reads them)
                if ((e = czk_v2_emit(d_streams, d_res, ns, d_wire.ptr, (uint32_t)SLOT_ALIGN, nullptr,
                                     (cz_frame_desc *)d_desc.ptr, qk)) != hipSuccess ||
                    (e = czk_open_desc((const cz_frame_desc *)d_desc.ptr, nullptr, sn, d_wire.ptr, d_plain.ptr, subkeys.ptr,
                                       (uint16_t *)d_status.ptr, (uint64_t *)d_nonces.ptr, qk)) != hipSuccess ||
                    (e = hipMemcpyAsync(h_plain.ptr, d_plain.ptr, spl, hipMemcpyDeviceToHost, qk)) != hipSuccess ||
                    (e = hipMemcpyAsync(h_status.ptr, d_status.ptr, (uint64_t)sn * 2, hipMemcpyDeviceToHost, qk)) !=
                        hipSuccess ||
                    (e = hipMemcpyAsync(h_nonces.ptr, d_nonces.ptr, (uint64_t)sn * 8, hipMemcpyDeviceToHost, qk)) !=
                        hipSuccess ||
                    (e = hipMemcpyAsync(h_meta.ptr, d_desc.ptr, (uint64_t)sn * sizeof(cz_frame_desc),
                                        hipMemcpyDeviceToHost, qk)) != hipSuccess) {
                    drain();
                    return hip_fail(e, "cz_engine: flush_in");
                }
            }
            for (uint32_t q = 0; q < ns; q++) {
                parsed[q].first = h_res[q].first;
                parsed[q].count = h_res[q].nframes;
                parsed[q].consumed = h_res[q].consumed;
                parsed[q].perr = h_res[q].rc;
            }
            scan_frames = sn;
        } else {
            std::vector<std::thread> th;
            for (size_t gi = 1; gi < groups.size(); gi++)
                th.emplace_back(parse, gi);
            if (!groups.empty())
                parse(0);
            for (std::thread &t : th)
                t.join();
        }
        pt.mark("parse");
        // 2. place the groups: absolute frame indices, slot offsets, segment-list offsets; size
        //    every buffer once
        uint32_t n = 0;
        uint64_t bslot = 0, pslot = 0, nseg = 0, ncomb = 0, npart = 0, nfan = 0;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            Group &g = groups[gi];
            GroupWork &w = gw[gi];
            w.foff = nfan;
            if (!w.runs.empty() || !w.sruns.empty())
                w.fbytes = w.frames.size() * sizeof(cz_fanin_sub) +
                           (w.runs.size() + w.sruns.size()) * sizeof(cz_fanin_run) + w.nfwave * sizeof(cz_fanout_wave) +
                           w.stiles * sizeof(cz_fanout_tile) + w.sjoins * sizeof(cz_fanout_join);
            nfan += w.fbytes;
            fanin_frames += w.nrouted;
            fanin_split_frames += w.nsrouted;
            g.fa = n;
            for (size_t q = g.pa; q < g.pb; q++)
                parsed[q].first += n;
            n += (uint32_t)w.frames.size();
            g.fb = n;
            g.pl0 = pslot;
            w.b0 = bslot;
            w.soff = nseg;
            w.coff = ncomb;
            w.woff = npart;
            bslot += w.bslot;
            pslot += w.pslot;
            nseg += w.nseg;
            ncomb += w.ncomb;
            npart += w.npart + w.spart;  // (the split runs' partial records behind the segment plan's)
            g.pl1 = pslot;
        }
        const uint64_t m_items = 0, m_desc = (uint64_t)n * sizeof(cz_v2_item),
                       m_seg = m_desc + (uint64_t)n * sizeof(cz_frame_desc),
                       m_comb = m_seg + nseg * sizeof(cz_segment), m_fanin = m_comb + ncomb * sizeof(cz_combine),
                       m_end = m_fanin + nfan;
        // (a device buffer that has to grow is reallocated here, which waits for the copies in
        //  flight; steady-state flushes reuse their buffers)
        if (n && ((e = d_in.reserve(bslot)) != hipSuccess || (e = d_plain.reserve(pslot)) != hipSuccess ||
                  (e = d_items.reserve((uint64_t)n * sizeof(cz_v2_item))) != hipSuccess ||
                  (e = d_status.reserve((uint64_t)n * 2)) != hipSuccess ||
                  (e = d_nonces.reserve((uint64_t)n * 8)) != hipSuccess ||
                  (e = d_desc.reserve((uint64_t)n * sizeof(cz_frame_desc))) != hipSuccess ||
                  (e = d_seg.reserve(std::max<uint64_t>(nseg, 1) * sizeof(cz_segment))) != hipSuccess ||
                  (e = d_comb.reserve(std::max<uint64_t>(ncomb, 1) * sizeof(cz_combine))) != hipSuccess ||
                  (e = d_work.reserve(std::max<uint64_t>(npart, 1) * 64)) != hipSuccess ||
                  // (the fan-out records' buffer of flush_out, which never runs beside flush_in)
                  (nfan && (e = d_subs.reserve(nfan)) != hipSuccess) ||
                  (e = h_plain.reserve(pslot)) != hipSuccess || (e = h_status.reserve((uint64_t)n * 2)) != hipSuccess ||
                  (e = h_nonces.reserve((uint64_t)n * 8)) != hipSuccess || (e = h_meta.reserve(m_end)) != hipSuccess))
            return hip_fail(e, "cz_engine: alloc");
        // the host-built arrays go straight into pinned staging (pageable sources would make each
        // H2D synchronous); descriptors stay there for the delivery step
        uint8_t *hm = (uint8_t *)h_meta.ptr;
        cz_v2_item *h_items = (cz_v2_item *)(hm + m_items);
        cz_frame_desc *h_desc = (cz_frame_desc *)(hm + m_desc);
        cz_segment *h_seg = (cz_segment *)(hm + m_seg);
        cz_combine *h_comb = (cz_combine *)(hm + m_comb);
        uint8_t *h_fanin = hm + m_fanin;
        pt.mark("place");
        // 3. per group, on its own host thread: descriptors -- bodies unpacked into aligned slots,
        //    each connection's frames chained by prev (group-relative indices, as the kernels get
        //    the group's descriptor array) -- and the segment plan.  This thread issues group g's
        //    metadata H2D, kernels and D2H as soon as its worker is done, while later groups are
        //    still being built.
        auto build = [&](size_t gi) {
            GroupWork &w = gw[gi];
            const Group &g = groups[gi];
            cz_v2_item *items = h_items + g.fa;
            cz_frame_desc *desc = h_desc + g.fa;
            uint64_t bs = w.b0, ps = g.pl0;
            for (size_t q = g.pa; q < g.pb; q++) {
                const Parsed &p = parsed[q];
                const Conn &c = conns[p.conn];
                for (uint32_t k = 0; k < p.count; k++) {
                    const uint32_t i = p.first - g.fa + k;
                    const cz_v2_frame &f = w.frames[i];
                    const uint64_t plen = f.size > CZ_MESSAGE_OVERHEAD ? f.size - CZ_MESSAGE_OVERHEAD : 0;
                    items[i] = {p.rx_off + f.body_off, bs, f.size, 0u};
                    desc[i] = {bs, ps, f.size, c.rx_key, c.peer_nonce, CZ_DESC_CHECK_NONCE, k ? (int32_t)(i - 1) : -1};
                    bs += round_up(std::max<uint64_t>(f.size, 1), SLOT_ALIGN);
                    ps += round_up(std::max<uint64_t>(plen, 1), SLOT_ALIGN);
                }
            }
            const uint32_t gn = g.fb - g.fa;
            if (w.bad_plan)
                return;
            if (w.runs.empty() && w.sruns.empty()) {
                plan_segments(desc, gn, 1, seg, w.sg.seg, w.sg.comb, w.sg.npart);
            } else {
                // Fan-in records of the routed frames, at the frame's index in the group (where its
                // status and nonce land): a connection's first frame checks against cnPeerNonce,
                // every later one against the wire nonce of its previous body's slot -- routed or
                // not.  The descriptors above stay whole: the prev chains of the frames left in the
                // segment plan resolve through them, and the delivery step reads them.
                cz_fanin_sub *h_isubs = (cz_fanin_sub *)(h_fanin + w.foff);
                cz_fanin_run *hr = (cz_fanin_run *)(h_isubs + gn);
                cz_fanin_run *hs = hr + w.runs.size();  // the split runs
                cz_fanout_wave *hw = (cz_fanout_wave *)(hs + w.sruns.size());
                cz_fanout_tile *ht = (cz_fanout_tile *)(hw + w.nfwave);
                cz_fanout_join *hj = (cz_fanout_join *)(ht + w.stiles);
                for (size_t q = g.pa; q < g.pb; q++) {
                    const Parsed &p = parsed[q];
                    const Conn &c = conns[p.conn];
                    for (uint32_t k = 0; k < p.count; k++) {
                        const uint32_t i = p.first - g.fa + k;
                        if (!w.routed[i])
                            continue;
                        h_isubs[i] = k ? cz_fanin_sub{desc[i - 1].in_off, c.rx_key,
                                                             CZ_FANIN_CHECK_NONCE | CZ_FANIN_FLOOR_IS_BODY}
                                              : cz_fanin_sub{c.peer_nonce, c.rx_key, CZ_FANIN_CHECK_NONCE};
                    }
                }
                for (size_t r = 0; r < w.runs.size() + w.sruns.size(); r++) {
                    const auto &run = r < w.runs.size() ? w.runs[r] : w.sruns[r - w.runs.size()];
                    const uint32_t first = run.first, size = desc[first].len;
                    hr[r] = {desc[first].in_off, round_up(size, SLOT_ALIGN), desc[first].out_off,
                             round_up(std::max<uint64_t>(size - CZ_MESSAGE_OVERHEAD, 1), SLOT_ALIGN), size, first,
                             run.second, 0u};
                }
                if (!w.runs.empty())
                    w.fregion = plan_fanin(hr, (uint32_t)w.runs.size(), d_in.ptr, d_plain.ptr, hw, w.fclass);
                if (!w.sruns.empty())
                    plan_fanin_split(hs, (uint32_t)w.sruns.size(), d_in.ptr, seg, ht, w.sclass, hj);
                // the segment plan of the frames that stay: planned over a packed copy of their
                // descriptors, then named by their index in the whole array
                std::vector<cz_frame_desc> rest;
                std::vector<uint32_t> index;
                rest.reserve(gn - w.nrouted - w.nsrouted);
                index.reserve(gn - w.nrouted - w.nsrouted);
                for (uint32_t i = 0; i < gn; i++)
                    if (!w.routed[i]) {
                        rest.push_back(desc[i]);
                        index.push_back(i);
                    }
                plan_segments(rest.data(), (uint32_t)rest.size(), 1, seg, w.sg.seg, w.sg.comb, w.sg.npart);
                for (cz_segment &sgm : w.sg.seg)
                    sgm.frame = index[sgm.frame];
                for (cz_combine &cb : w.sg.comb)
                    cb.frame = index[cb.frame];
            }
            w.sg.nseg = (uint32_t)w.sg.seg.size();
            w.sg.ncomb = (uint32_t)w.sg.comb.size();
            if (w.sg.nseg != w.nseg || w.sg.ncomb != w.ncomb || w.sg.npart != w.npart) {
                w.bad_plan = true;
                return;
            }
            memcpy(h_seg + w.soff, w.sg.seg.data(), (uint64_t)w.sg.nseg * sizeof(cz_segment));
            memcpy(h_comb + w.coff, w.sg.comb.data(), (uint64_t)w.sg.ncomb * sizeof(cz_combine));
        };
        auto issue = [&](size_t gi) -> hipError_t {
            const Group &g = groups[gi];
            const GroupWork &w = gw[gi];
            const uint32_t gn = g.fb - g.fa;
            if (gn == 0)
                return hipSuccess;
            cz_frame_desc *dd = (cz_frame_desc *)d_desc.ptr + g.fa;
            cz_segment *dsg = (cz_segment *)d_seg.ptr + w.soff;
            cz_combine *dcb = (cz_combine *)d_comb.ptr + w.coff;
            const uint32_t nr = (uint32_t)w.runs.size(), nsr = (uint32_t)w.sruns.size();
            // the group's fan-in block on the device: records, runs, waves, tiles, joins, laid out as in the staging
            const cz_fanin_sub *dis = (const cz_fanin_sub *)((const uint8_t *)d_subs.ptr + w.foff);
            const cz_fanin_run *dir = (const cz_fanin_run *)(dis + gn);
            const cz_fanin_run *dsr = dir + nr;
            const cz_fanout_wave *diw = (const cz_fanout_wave *)(dsr + nsr);
            const cz_fanout_tile *dst = (const cz_fanout_tile *)(diw + w.nfwave);
            const cz_fanout_join *dsj = (const cz_fanout_join *)(dst + w.stiles);
            // first record used
            const uint64_t sub_a = (uint64_t)std::min(nr ? w.runs.front().first : UINT32_MAX,
                                                      nsr ? w.sruns.front().first : UINT32_MAX) * sizeof(cz_fanin_sub);
            hipError_t r;
            // (a) metadata stream: the group's descriptors / items / segment lists
            if ((r = hipMemcpyAsync((cz_v2_item *)d_items.ptr + g.fa, h_items + g.fa, (uint64_t)gn * sizeof(cz_v2_item),
                                    hipMemcpyHostToDevice, qm)) != hipSuccess ||
                (r = hipMemcpyAsync(dd, h_desc + g.fa, (uint64_t)gn * sizeof(cz_frame_desc), hipMemcpyHostToDevice,
                                    qm)) != hipSuccess ||
                (w.sg.nseg && (r = hipMemcpyAsync(dsg, h_seg + w.soff, (uint64_t)w.sg.nseg * sizeof(cz_segment),
                                                  hipMemcpyHostToDevice, qm)) != hipSuccess) ||
                (w.sg.ncomb && (r = hipMemcpyAsync(dcb, h_comb + w.coff, (uint64_t)w.sg.ncomb * sizeof(cz_combine),
                                                   hipMemcpyHostToDevice, qm)) != hipSuccess) ||
                // (one copy for the group's fan-in block, from the first routed frame's record on)
                ((nr || nsr) && (r = hipMemcpyAsync((uint8_t *)d_subs.ptr + w.foff + sub_a, h_fanin + w.foff + sub_a,
                                           w.fbytes - sub_a, hipMemcpyHostToDevice, qm)) != hipSuccess) ||
                (qm != qk && (r = hipEventRecord(evm[gi], qm)) != hipSuccess))
                return r;
            // (b) compute stream: once the group's bytes and metadata landed, unpack + open;
            // (c) D2H stream
            if ((qh != qk && (r = hipStreamWaitEvent(qk, ev[gi], 0)) != hipSuccess) ||
                (qm != qk && (r = hipStreamWaitEvent(qk, evm[gi], 0)) != hipSuccess) ||
                (r = czk_v2_copy((const cz_v2_item *)d_items.ptr + g.fa, gn, d_wire.ptr, d_in.ptr, qk)) != hipSuccess ||
                // the group's fan-in runs in one call (records, statuses and nonces by frame index in the
                // group), then the segment plan of the frames that stay
                (nr && (r = czk_open_fanin_runs(dir, diw, w.fclass, w.fregion, d_in.ptr, dis, subkeys.ptr, d_plain.ptr,
                                                (uint16_t *)d_status.ptr + g.fa, (uint64_t *)d_nonces.ptr + g.fa,
                                                qk)) != hipSuccess) ||
                // ... its split runs on the connection x segment grid, at the flush's own segment length
                (nsr && (r = czk_open_fanin_split(dsr, dst, w.sclass, dsj, (uint32_t)w.sjoins, d_in.ptr, dis, subkeys.ptr,
                                                  d_plain.ptr, (uint8_t *)d_work.ptr + 64 * (w.woff + w.npart),
                                                  (uint16_t *)d_status.ptr + g.fa, (uint64_t *)d_nonces.ptr + g.fa,
                                                  qk)) != hipSuccess) ||
                (w.sg.nseg &&
                 (r = czk_open_segments(dd, dsg, w.sg.nseg, dcb, w.sg.ncomb, d_in.ptr, d_plain.ptr, subkeys.ptr,
                                        (uint8_t *)d_work.ptr + 64 * w.woff, (uint16_t *)d_status.ptr + g.fa,
                                        (uint64_t *)d_nonces.ptr + g.fa, qk)) != hipSuccess) ||
                (qo != qk && ((r = hipEventRecord(evk[gi], qk)) != hipSuccess ||
                              (r = hipStreamWaitEvent(qo, evk[gi], 0)) != hipSuccess)) ||
                (r = hipMemcpyAsync((uint8_t *)h_plain.ptr + g.pl0, (uint8_t *)d_plain.ptr + g.pl0, g.pl1 - g.pl0,
                                    hipMemcpyDeviceToHost, qo)) != hipSuccess ||
                (r = hipMemcpyAsync((uint16_t *)h_status.ptr + g.fa, (uint16_t *)d_status.ptr + g.fa, (uint64_t)gn * 2,
                                    hipMemcpyDeviceToHost, qo)) != hipSuccess ||
                (r = hipMemcpyAsync((uint64_t *)h_nonces.ptr + g.fa, (uint64_t *)d_nonces.ptr + g.fa, (uint64_t)gn * 8,
                                    hipMemcpyDeviceToHost, qo)) != hipSuccess)
                return r;
            return hipSuccess;
        };
        if (n) {
            std::vector<std::thread> th;
            for (size_t gi = 1; gi < groups.size(); gi++)
                th.emplace_back(build, gi);
            build(0);
            e = hipSuccess;
            bool bad = false;
            for (size_t gi = 0; gi < groups.size(); gi++) {
                if (gi)
                    th[gi - 1].join();
                bad = bad || gw[gi].bad_plan;
                if (!bad && e == hipSuccess)
                    e = issue(gi);  // after a failure: join the rest, issue nothing more
            }
            if (bad)
                return fail(CZ_EINVAL, "cz_engine: internal error, segment plan differs from its count");
            if (e != hipSuccess)
                return hip_fail(e, "cz_engine: flush_in");
        }
        const hipStream_t used[4] = {qh, qk, qo, qm};
        for (int i = 0; i < 4; i++)
            if (std::find(used, used + i, used[i]) == used + i && (e = hipStreamSynchronize(used[i])) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_in");
        pt.mark("h2d+kernels+d2h");
        // 3. deliver in order per connection, up to the first failure (decodeAndPush returns false)
        const uint16_t *st = (const uint16_t *)h_status.ptr;
        const uint64_t *nn = (const uint64_t *)h_nonces.ptr;
        for (const Parsed &p : parsed) {
            Conn &c = conns[p.conn];
            bool failed = false;
            for (uint32_t k = 0; k < p.count; k++) {
                const uint32_t i = p.first + k;
                const uint32_t status = st[i] & 0xffu;
                if (status != CZ_STATUS_OK) {
                    if (status == CZ_STATUS_CRYPTO)  // the nonce passed the replay check: cnPeerNonce = nonce
                        c.peer_nonce = nn[i];        // precedes openAfternm (CurveClientMechanism.java:193)
                    c.error = CZ_EPROTO;
                    c.event = event_for(status, c.server);
                    failed = true;
                    break;
                }
                c.peer_nonce = nn[i];
                const uint32_t fl = st[i] >> 8;
                int mf = 0;
                if (fl & 0x01)
                    mf |= CZ_MSG_MORE;
                if (fl & 0x02)
                    mf |= CZ_MSG_COMMAND;
                c.in_msgs.push_back((uint32_t)in_msgs.size());
                in_msgs.push_back({h_desc[i].out_off, h_desc[i].len - CZ_MESSAGE_OVERHEAD, mf});
            }
            if (failed) {
                c.rx_len = 0;
                continue;
            }
            // keep the partial frame for the next read
            if (p.consumed) {
                memmove(c.rx.ptr, (uint8_t *)c.rx.ptr + p.consumed, c.rx_len - p.consumed);
                c.rx_len -= p.consumed;
            }
            if (p.perr) {  // V2Decoder error after the good frames: StreamEngine error(PROTOCOL)
                c.error = p.perr;
                c.event = 0;
                c.rx_len = 0;
            }
        }
        pt.mark("deliver");
        return CZ_OK;
    }

    // Forward routes (header section 3j): Proxy.forward for every routed connection at once, without delivery.
    // On one stream, as the scanned flush: the sources' received bytes go over as they lie (one DMA per run of
    // neighbours in the receive blocks), one cz_v2_stream and one cz_fanout_sub per route follow, the device
    // scans and places the streams, the totals come back (the one extra synchronisation, which sizes the
    // per-frame buffers), and then cz_relay_streams' chain runs IN PLACE: emit with materialised floors, one
    // relay lane per frame, the cut.  The receive regions lie a region's spare capacity apart, so k_v2_copy
    // (one item per route) packs the streams densely before they come back.  What comes back is the wire bytes,
    // now the destinations' outbound streams, and 32 bytes per route; no per-frame record crosses PCIe in
    // either direction.
    int flush_forward()
    {
        PhaseTimer pt("flush_forward");
        forward_frames = 0;
        for (Conn &c : conns)
            c.fwd_off = c.fwd_len = 0;
        struct Route {
            uint32_t from, to;
            uint64_t off;    // where the source's received bytes start in d_wire
            uint64_t dense;  // ... and in the packed copy that comes back into h_fwd
        };
        std::vector<Route> rt;
        for (size_t ci = 0; ci < conns.size(); ci++) {
            const int t = routes.dest((int)ci);
            const Conn &c = conns[ci];
            // (a failed destination: the source's bytes stay where they are)
            if (t < 0 || c.error || c.rx_len == 0 || conns[(size_t)t].error)
                continue;
            if (c.rx_len > 0xffffffffull)
                return fail(CZ_EINVAL, "cz_engine: more than 4 GiB received on routed connection %zu in one flush", ci);
            rt.push_back({(uint32_t)ci, (uint32_t)t, 0, 0});
        }
        const uint32_t ns = (uint32_t)rt.size();
        if (ns == 0)
            return CZ_OK;
        uint64_t dense = 0;
        for (Route &r : rt) {
            r.dense = dense;
            dense += conns[r.from].rx_len;
        }
        // spans, as flush_in (place_in_spans): the sources in address order
        std::vector<Span> spans;
        uint64_t total = 0;
        {
            std::vector<uint32_t> order(ns);
            for (uint32_t q = 0; q < ns; q++)
                order[q] = q;
            std::sort(order.begin(), order.end(),
                      [&](uint32_t x, uint32_t y) { return conns[rt[x].from].rx.ptr < conns[rt[y].from].rx.ptr; });
            uint32_t blk = 0;
            for (uint32_t q : order) {
                const Conn &c = conns[rt[q].from];
                rt[q].off = place_in_spans(spans, 0, blk, total, c.rx, c.rx_len);
            }
        }
        // one staging block: streams | outbound records | packing items | scan results | totals | cut results
        const uint64_t o_to = (uint64_t)ns * sizeof(cz_v2_stream), o_items = o_to + (uint64_t)ns * sizeof(cz_fanout_sub),
                       o_res = o_items + (uint64_t)ns * sizeof(cz_v2_item),
                       o_tot = o_res + (uint64_t)ns * sizeof(cz_v2_stream_result), o_cut = o_tot + sizeof(cz_v2_totals),
                       o_end = o_cut + (uint64_t)ns * sizeof(cz_relay_stream_result);
        hipError_t e;
        // (+ 16: a frame's replay floor is read at bytes [8, 16) of the frame before it where they lie)
        if ((e = d_wire.reserve(total + 16)) != hipSuccess || (e = d_body.reserve(dense)) != hipSuccess ||
            (e = h_fwd.reserve(dense)) != hipSuccess ||
            (e = h_scan.reserve(o_end)) != hipSuccess || (e = d_scan.reserve(o_end)) != hipSuccess)
            return hip_fail(e, "cz_engine: alloc");
        uint8_t *hs = (uint8_t *)h_scan.ptr, *ds = (uint8_t *)d_scan.ptr;
        cz_v2_stream *h_streams = (cz_v2_stream *)hs;
        cz_fanout_sub *h_to = (cz_fanout_sub *)(hs + o_to);
        cz_v2_item *h_items = (cz_v2_item *)(hs + o_items);
        for (uint32_t q = 0; q < ns; q++) {
            const Conn &f = conns[rt[q].from], &t = conns[rt[q].to];
            h_streams[q] = {rt[q].off, f.rx_len, f.peer_nonce, f.rx_key, 0u};
            h_to[q] = {t.nonce, t.tx_key, 0u};
            h_items[q] = {rt[q].off, rt[q].dense, (uint32_t)f.rx_len, 0u};
        }
        const cz_v2_stream *d_streams = (const cz_v2_stream *)ds;
        const cz_fanout_sub *d_to = (const cz_fanout_sub *)(ds + o_to);
        cz_v2_stream_result *d_res = (cz_v2_stream_result *)(ds + o_res);
        cz_relay_stream_result *d_cut = (cz_relay_stream_result *)(ds + o_cut);
        const cz_v2_stream_result *h_res = (const cz_v2_stream_result *)(hs + o_res);
        const cz_v2_totals *h_tot = (const cz_v2_totals *)(hs + o_tot);
        const cz_relay_stream_result *h_cut = (const cz_relay_stream_result *)(hs + o_cut);
        const hipStream_t qk = ps[1];
        for (const Span &sp : spans)
            if ((e = hipMemcpyAsync((uint8_t *)d_wire.ptr + sp.dev, sp.src, sp.len, hipMemcpyHostToDevice, qk)) !=
                hipSuccess)
                return hip_fail(e, "cz_engine: H2D");
        if ((e = hipMemcpyAsync(ds, hs, o_res, hipMemcpyHostToDevice, qk)) != hipSuccess ||
            (e = czk_v2_scan(d_streams, ns, d_wire.ptr, -1, 1u, d_res, (cz_v2_totals *)(ds + o_tot), qk)) != hipSuccess ||
            (e = hipMemcpyAsync(hs + o_res, ds + o_res, o_cut - o_res, hipMemcpyDeviceToHost, qk)) != hipSuccess ||
            (e = hipStreamSynchronize(qk)) != hipSuccess)
            return hip_fail(e, "cz_engine: flush_forward scan");
        pt.mark("h2d+scan");
        if (h_tot->nframes > 0x7fffffffull)
            return fail(CZ_EINVAL, "cz_engine: more than 2^31 - 1 received frames in one flush");
        const uint32_t sn = (uint32_t)h_tot->nframes;
        if (sn) {
            if ((e = d_desc.reserve((uint64_t)sn * sizeof(cz_frame_desc))) != hipSuccess ||
                (e = d_subs.reserve((uint64_t)sn * sizeof(cz_fanout_sub))) != hipSuccess ||
                (e = d_status.reserve((uint64_t)sn * 2)) != hipSuccess ||
                (e = d_nonces.reserve((uint64_t)sn * 8)) != hipSuccess)
                return hip_fail(e, "cz_engine: alloc");
            if ((e = czk_v2_emit_relay(d_streams, d_to, d_res, ns, d_wire.ptr, d_wire.ptr, (cz_frame_desc *)d_desc.ptr,
                                       (cz_fanout_sub *)d_subs.ptr, qk)) != hipSuccess ||
                (e = czk_relay_desc((const cz_frame_desc *)d_desc.ptr, (const cz_fanout_sub *)d_subs.ptr, nullptr, sn,
                                    d_wire.ptr, d_wire.ptr, subkeys.ptr, (uint16_t *)d_status.ptr,
                                    (uint64_t *)d_nonces.ptr, qk)) != hipSuccess)
                return hip_fail(e, "cz_engine: flush_forward");
        }
        // (no frame at all: every lane of the cut writes the empty result without reading a per-frame record)
        if ((e = czk_relay_cut(d_streams, d_res, ns, (const cz_frame_desc *)d_desc.ptr, (const uint16_t *)d_status.ptr,
                               (const uint64_t *)d_nonces.ptr, d_cut, qk)) != hipSuccess ||
            (e = hipMemcpyAsync(hs + o_cut, d_cut, o_end - o_cut, hipMemcpyDeviceToHost, qk)) != hipSuccess)
            return hip_fail(e, "cz_engine: flush_forward");
        if (sn && ((e = czk_v2_copy((const cz_v2_item *)(ds + o_items), ns, d_wire.ptr, d_body.ptr, qk)) != hipSuccess ||
                   (e = hipMemcpyAsync(h_fwd.ptr, d_body.ptr, dense, hipMemcpyDeviceToHost, qk)) != hipSuccess))
            return hip_fail(e, "cz_engine: D2H");
        if ((e = hipStreamSynchronize(qk)) != hipSuccess)
            return hip_fail(e, "cz_engine: flush_forward");
        pt.mark("relay+d2h");
        // what leaves, and the two ends' state: the source as flush_in leaves a receiver, the destination as
        // flush_out leaves a sender of as many frames as were scanned (a rejected frame consumed its counter)
        for (uint32_t q = 0; q < ns; q++) {
            Conn &f = conns[rt[q].from], &t = conns[rt[q].to];
            const cz_v2_stream_result &sr = h_res[q];
            const cz_relay_stream_result &cr = h_cut[q];
            f.fwd_off = rt[q].dense;
            f.fwd_len = cr.ok_bytes;
            f.peer_nonce = cr.peer_nonce;
            t.nonce += sr.nframes;
            forward_frames += cr.ok_frames;
            if (cr.fail_status != CZ_STATUS_OK) {
                f.error = CZ_EPROTO;
                f.event = event_for(cr.fail_status, f.server);
                f.rx_len = 0;
                continue;
            }
            if (sr.consumed) {  // keep the partial frame for the next read
                memmove(f.rx.ptr, (uint8_t *)f.rx.ptr + sr.consumed, f.rx_len - sr.consumed);
                f.rx_len -= sr.consumed;
            }
            if (sr.rc) {  // V2Decoder error after the good frames: StreamEngine error(PROTOCOL)
                f.error = sr.rc;
                f.event = 0;
                f.rx_len = 0;
            }
        }
        pt.mark("deliver");
        return CZ_OK;
    }
};

namespace czi {

int engine_device(const cz_engine *e) { return e->device; }

// Bulk session hand-over, the add side.  What a loop of cz_engine_add_conn does per connection
// (hipMalloc, H2D, two k_subkeys launches, memset, synchronise, hipFree) is one chain for the batch:
//   grow the subkey table once | H2D of the job records (and, staged, of the precoms) |
//   k_session_subkeys | wipe the device staging | synchronise | wipe the pinned staging
// Ids and key slots are planned first, exactly as the loop would hand them out (free_ids from the
// back, then new ids in order), and the engine's tables change only after the synchronisation: a
// failure hands out nothing.
int engine_add_sessions(cz_engine *e, const char *where, uint32_t count, const SessionItem *items, const void *d_base,
                        int32_t *ids)
{
    uint32_t nv = 0;
    for (uint32_t i = 0; i < count; i++) {
        ids[i] = CZ_EINVAL;
        nv += items[i].ok ? 1u : 0u;
    }
    if (nv == 0)
        return CZ_OK;
    auto all_failed = [&](int rc) {
        for (uint32_t i = 0; i < count; i++)
            ids[i] = rc;
        return rc;
    };
    const uint32_t nfree = (uint32_t)e->free_ids.size();
    const uint32_t nnew = nv - std::min(nv, nfree);
    if (nnew > (0x7fffffffu - e->nkeys) / 2 || e->conns.size() + nnew > 0x7fffffffu)
        return all_failed(fail(CZ_ENOMEM, "%s: %u more connections exceed the id range", where, nnew));
    const bool staged = d_base == nullptr;
    const uint64_t keys_b = staged ? 32ull * nv : 0, total = keys_b + (uint64_t)nv * sizeof(cz_session_job);
    hipError_t he;
    if ((he = hipSetDevice(e->device)) != hipSuccess || (nnew && (he = e->grow_keys(e->nkeys + 2 * nnew)) != hipSuccess) ||
        (he = e->d_stage.reserve(total)) != hipSuccess || (he = e->h_stage.reserve(total)) != hipSuccess)
        return all_failed(hip_fail(he, where));
    uint8_t *hs = (uint8_t *)e->h_stage.ptr, *ds = (uint8_t *)e->d_stage.ptr;
    cz_session_job *jobs = (cz_session_job *)(hs + keys_b);
    uint32_t fr = nfree, nk = e->nkeys, j = 0;
    int32_t next_id = (int32_t)e->conns.size();
    for (uint32_t i = 0; i < count; i++) {
        if (!items[i].ok)
            continue;
        uint32_t tx, rx;
        if (fr) {  // a removed connection's id and key slots
            ids[i] = e->free_ids[--fr];
            tx = e->conns[(size_t)ids[i]].tx_key;
            rx = e->conns[(size_t)ids[i]].rx_key;
        } else {
            ids[i] = next_id++;
            tx = nk;
            rx = nk + 1;
            nk += 2;
        }
        if (staged)
            memcpy(hs + 32ull * j, items[i].h_key, 32);
        jobs[j] = {staged ? 32ull * j : items[i].src_off, tx, rx, items[i].server ? 1u : 0u, 0u};
        j++;
    }
    if ((he = hipMemcpyAsync(ds, hs, total, hipMemcpyHostToDevice, e->stream)) != hipSuccess ||
        (he = czk_session_subkeys((const cz_session_job *)(ds + keys_b), nv, staged ? ds : d_base, e->subkeys.ptr,
                                  e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(ds, 0, total, e->stream)) != hipSuccess ||
        (he = hipStreamSynchronize(e->stream)) != hipSuccess) {
        // nothing is handed out: the table entries a lane may have written and the staging are wiped
        uint8_t *table = (uint8_t *)e->subkeys.ptr;
        if (nk > e->nkeys)
            (void)hipMemsetAsync(table + 32ull * e->nkeys, 0, 32ull * (nk - e->nkeys), e->stream);
        for (uint32_t k = 0; k < nv; k++)
            if (jobs[k].tx_key < e->nkeys) {
                (void)hipMemsetAsync(table + 32ull * jobs[k].tx_key, 0, 32, e->stream);
                (void)hipMemsetAsync(table + 32ull * jobs[k].rx_key, 0, 32, e->stream);
            }
        (void)hipMemsetAsync(ds, 0, total, e->stream);
        (void)hipStreamSynchronize(e->stream);
        secure_wipe(hs, keys_b);
        return all_failed(hip_fail(he, where));
    }
    secure_wipe(hs, keys_b);
    j = 0;
    for (uint32_t i = 0; i < count; i++) {
        if (!items[i].ok)
            continue;
        Conn c;
        c.server = items[i].server != 0;
        c.tx_key = jobs[j].tx_key;
        c.rx_key = jobs[j].rx_key;
        c.nonce = items[i].nonce;
        c.peer_nonce = items[i].peer_nonce;
        j++;
        if ((size_t)ids[i] < e->conns.size())
            e->conns[(size_t)ids[i]] = std::move(c);
        else
            e->conns.push_back(std::move(c));
    }
    e->free_ids.resize(fr);
    e->nkeys = nk;
    return CZ_OK;
}

}  // namespace czi

extern "C" {

int cz_engine_create(cz_engine **out, uint64_t arena_bytes, int device)
{
    if (!out)
        return fail(CZ_EINVAL, "cz_engine_create: null pointer");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(CZ_EHIP, "no HIP device available (the CURVE path runs only on the GPU)");
    cz_engine *e = new cz_engine();
    e->device = device;
    hipError_t he;
    if ((he = hipSetDevice(device)) != hipSuccess ||
        (he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess ||
        (he = hipStreamCreateWithFlags(&e->ps[0], hipStreamNonBlocking)) != hipSuccess ||
        (he = hipStreamCreateWithFlags(&e->ps[1], hipStreamNonBlocking)) != hipSuccess ||
        (he = hipStreamCreateWithFlags(&e->ps[2], hipStreamNonBlocking)) != hipSuccess ||
        (he = e->arena.reserve(std::max<uint64_t>(arena_bytes, 4096))) != hipSuccess) {
        delete e;
        return hip_fail(he, "cz_engine_create");
    }
    e->arena_cap = e->arena.cap;
    *out = e;
    return CZ_OK;
}

void cz_engine_destroy(cz_engine *e) { delete e; }

int cz_engine_add_conn(cz_engine *e, int as_server, const uint8_t precom[32], uint64_t cn_nonce,
                       uint64_t cn_peer_nonce)
{
    if (!e || !precom)
        return fail(CZ_EINVAL, "cz_engine_add_conn: null pointer");
    hipError_t he;
    // a removed connection's id and subkey slots first, else two new table slots
    const bool reuse = !e->free_ids.empty();
    if ((he = hipSetDevice(e->device)) != hipSuccess || (!reuse && (he = e->grow_keys(e->nkeys + 2)) != hipSuccess))
        return hip_fail(he, "cz_engine_add_conn");
    void *dk = nullptr;
    if ((he = hipMalloc(&dk, 32)) != hipSuccess)
        return hip_fail(he, "hipMalloc");
    Conn c;
    c.server = as_server != 0;
    c.tx_key = reuse ? e->conns[(size_t)e->free_ids.back()].tx_key : e->nkeys;
    c.rx_key = reuse ? e->conns[(size_t)e->free_ids.back()].rx_key : e->nkeys + 1;
    c.nonce = cn_nonce;
    c.peer_nonce = cn_peer_nonce;
    uint8_t *table = (uint8_t *)e->subkeys.ptr;
    const int tx = c.server ? CZ_DIR_S2C : CZ_DIR_C2S;
    const int rx = c.server ? CZ_DIR_C2S : CZ_DIR_S2C;
    if ((he = hipMemcpyAsync(dk, precom, 32, hipMemcpyHostToDevice, e->stream)) != hipSuccess ||
        (he = czk_subkeys(dk, table + 32ull * c.tx_key, 1, prefix_for(tx), e->stream)) != hipSuccess ||
        (he = czk_subkeys(dk, table + 32ull * c.rx_key, 1, prefix_for(rx), e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(dk, 0, 32, e->stream)) != hipSuccess || (he = hipStreamSynchronize(e->stream)) != hipSuccess) {
        (void)hipFree(dk);
        return hip_fail(he, "cz_engine_add_conn: subkeys");
    }
    (void)hipFree(dk);
    if (reuse) {
        const int id = e->free_ids.back();
        e->free_ids.pop_back();
        e->conns[(size_t)id] = std::move(c);
        return id;
    }
    e->nkeys += 2;
    e->conns.push_back(std::move(c));
    return (int)e->conns.size() - 1;
}

// StreamEngine teardown (unplug / error, StreamEngine.java:334-370,1116-1131) of an attached
// connection: its queued messages leave the next flush, its received bytes and the payloads of the
// last flush_in are dropped, its subkeys are wiped on the device, and its id and key slots are
// reused by the next cz_engine_add_conn -- a long-lived IO thread with connection churn keeps a
// bounded engine.
int cz_engine_remove_conn(cz_engine *e, int conn)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_remove_conn: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    hipError_t he;
    uint8_t *table = (uint8_t *)e->subkeys.ptr;
    if ((he = hipSetDevice(e->device)) != hipSuccess ||
        (he = hipMemsetAsync(table + 32ull * c->tx_key, 0, 32, e->stream)) != hipSuccess ||
        (he = hipMemsetAsync(table + 32ull * c->rx_key, 0, 32, e->stream)) != hipSuccess ||
        (he = hipStreamSynchronize(e->stream)) != hipSuccess)
        return hip_fail(he, "cz_engine_remove_conn");
    e->pend.erase(std::remove_if(e->pend.begin(), e->pend.end(), [conn](const OutMsg &m) { return (int)m.conn == conn; }),
                  e->pend.end());
    if (c->rx.ptr) {
        explicit_bzero(c->rx.ptr, c->rx_len);
        e->rxpool.free_list.push_back(c->rx);
    }
    Conn dead;
    dead.tx_key = c->tx_key;
    dead.rx_key = c->rx_key;
    dead.removed = true;
    *c = std::move(dead);
    e->routes.drop(conn);
    e->free_ids.push_back(conn);
    return CZ_OK;
}

int cz_engine_add_conns(cz_engine *e, uint32_t count, const uint8_t *as_server, const uint8_t *precoms,
                        const uint64_t *cn_nonce, const uint64_t *cn_peer_nonce, int32_t *ids)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_add_conns: null pointer");
    if (count == 0)
        return CZ_OK;
    for (uint32_t i = 0; ids && i < count; i++)
        ids[i] = CZ_EINVAL;
    if (!precoms || !cn_nonce || !cn_peer_nonce || !ids)
        return fail(CZ_EINVAL, "cz_engine_add_conns: null pointer");
    std::vector<SessionItem> items(count);
    for (uint32_t i = 0; i < count; i++)
        items[i] = {1, (uint8_t)(as_server && as_server[i] ? 1 : 0), 0, precoms + 32ull * i, cn_nonce[i], cn_peer_nonce[i]};
    return engine_add_sessions(e, "cz_engine_add_conns", count, items.data(), nullptr, ids);
}

// cz_engine_remove_conn for a list: the subkeys of every connection named are wiped by one
// k_scatter_wipe launch behind one H2D of their table indices, with one synchronisation; the host
// side of each removal follows in list order, so free_ids ends as the loop leaves it.
int cz_engine_remove_conns(cz_engine *e, uint32_t count, const int *conns, int32_t *rcs)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_remove_conns: null pointer");
    if (count == 0)
        return CZ_OK;
    if (!conns || !rcs)
        return fail(CZ_EINVAL, "cz_engine_remove_conns: null pointer");
    hipError_t he;
    if ((he = hipSetDevice(e->device)) != hipSuccess || (he = e->h_stage.reserve(8ull * count)) != hipSuccess ||
        (he = e->d_stage.reserve(8ull * count)) != hipSuccess) {
        std::fill(rcs, rcs + count, (int32_t)CZ_EHIP);
        return hip_fail(he, "cz_engine_remove_conns");
    }
    // a connection is marked as it is named: a second mention finds it gone, as in the loop
    uint32_t *idx = (uint32_t *)e->h_stage.ptr;
    std::vector<int> hit;
    for (uint32_t i = 0; i < count; i++) {
        Conn *c = e->conn(conns[i]);
        rcs[i] = c ? CZ_OK : CZ_EINVAL;
        if (!c)
            continue;
        idx[2 * hit.size()] = c->tx_key;
        idx[2 * hit.size() + 1] = c->rx_key;
        c->removed = true;
        hit.push_back(conns[i]);
    }
    if (hit.empty())
        return CZ_OK;
    const uint32_t nidx = 2 * (uint32_t)hit.size();
    if ((he = hipMemcpyAsync(e->d_stage.ptr, idx, 4ull * nidx, hipMemcpyHostToDevice, e->stream)) != hipSuccess ||
        (he = czk_scatter_wipe(e->subkeys.ptr, (const uint32_t *)e->d_stage.ptr, nidx, 32, 0, e->stream)) != hipSuccess ||
        (he = hipStreamSynchronize(e->stream)) != hipSuccess) {
        (void)hipStreamSynchronize(e->stream);
        for (int id : hit)
            e->conns[(size_t)id].removed = false;
        std::fill(rcs, rcs + count, (int32_t)CZ_EHIP);
        return hip_fail(he, "cz_engine_remove_conns");
    }
    e->pend.erase(std::remove_if(e->pend.begin(), e->pend.end(),
                                 [e](const OutMsg &m) { return e->conns[m.conn].removed; }),
                  e->pend.end());
    for (int id : hit) {
        Conn &c = e->conns[(size_t)id];
        if (c.rx.ptr) {
            explicit_bzero(c.rx.ptr, c.rx_len);
            e->rxpool.free_list.push_back(c.rx);
        }
        Conn dead;
        dead.tx_key = c.tx_key;
        dead.rx_key = c.rx_key;
        dead.removed = true;
        c = std::move(dead);
        e->routes.drop(id);
        e->free_ids.push_back(id);
    }
    return CZ_OK;
}

void *cz_engine_msg_alloc(cz_engine *e, uint32_t len)
{
    if (!e)
        return nullptr;
    const uint64_t off = round_up(e->arena_used, 16);
    if (off + len > e->arena_cap)
        return nullptr;
    e->arena_used = off + len;
    return (uint8_t *)e->arena.ptr + off;
}

int cz_engine_send(cz_engine *e, int conn, const void *payload, uint32_t len, int msg_flags)
{
    if (!e || (len && !payload))
        return fail(CZ_EINVAL, "cz_engine_send: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (c->error)
        return fail(c->error, "cz_engine_send: connection %d has failed", conn);
    if (len > (uint32_t)CZ_MESSAGE_MAX)
        return fail(CZ_EMSGSIZE, "cz_engine_send: %u-byte payload exceeds CZ_MESSAGE_MAX", len);
    const uint8_t *base = (const uint8_t *)e->arena.ptr;
    const uint8_t *p = (const uint8_t *)payload;
    uint64_t off;
    if (len && p >= base && p + len <= base + e->arena_used) {
        off = (uint64_t)(p - base);  // allocated by cz_engine_msg_alloc: no copy
    } else {
        uint8_t *dst = (uint8_t *)cz_engine_msg_alloc(e, len);
        if (!dst)
            return fail(CZ_ENOMEM, "cz_engine_send: arena full (%llu bytes), flush first",
                        (unsigned long long)e->arena_cap);
        if (len)
            memcpy(dst, p, len);
        off = (uint64_t)(dst - base);
    }
    uint32_t fl = 0;
    if (msg_flags & CZ_MSG_MORE)
        fl |= 0x01;
    if (msg_flags & CZ_MSG_COMMAND)
        fl |= 0x02;
    e->pend.push_back({(uint32_t)conn, off, len, fl});
    return CZ_OK;
}

int cz_engine_publish(cz_engine *e, const int *conns, uint32_t nconn, const void *payload, uint32_t len,
                      int msg_flags, uint32_t *queued)
{
    if (queued)
        *queued = 0;
    if (!e || (nconn && !conns) || (len && !payload))
        return fail(CZ_EINVAL, "cz_engine_publish: null pointer");
    // everything is checked before anything is queued
    uint32_t live = 0;
    for (uint32_t k = 0; k < nconn; k++) {
        const Conn *c = e->conn(conns[k]);
        if (!c)
            return CZ_EINVAL;
        live += c->error ? 0u : 1u;  // a failed connection is skipped, as Dist.write drops its pipe
    }
    if (len > (uint32_t)CZ_MESSAGE_MAX)
        return fail(CZ_EMSGSIZE, "cz_engine_publish: %u-byte payload exceeds CZ_MESSAGE_MAX", len);
    if (live == 0)
        return CZ_OK;
    const uint8_t *base = (const uint8_t *)e->arena.ptr;
    const uint8_t *p = (const uint8_t *)payload;
    uint64_t off;
    if (len && p >= base && p + len <= base + e->arena_used) {
        off = (uint64_t)(p - base);  // allocated by cz_engine_msg_alloc: no copy
    } else {
        uint8_t *dst = (uint8_t *)cz_engine_msg_alloc(e, len);  // staged once for every subscriber
        if (!dst)
            return fail(CZ_ENOMEM, "cz_engine_publish: arena full (%llu bytes), flush first",
                        (unsigned long long)e->arena_cap);
        if (len)
            memcpy(dst, p, len);
        off = (uint64_t)(dst - base);
    }
    uint32_t fl = 0;
    if (msg_flags & CZ_MSG_MORE)
        fl |= 0x01;
    if (msg_flags & CZ_MSG_COMMAND)
        fl |= 0x02;
    if (++e->pub_seq == 0)
        e->pub_seq = 1;
    for (uint32_t k = 0; k < nconn; k++)
        if (!e->conns[(size_t)conns[k]].error)
            e->pend.push_back({(uint32_t)conns[k], off, len, fl, e->pub_seq});
    if (queued)
        *queued = live;
    return CZ_OK;
}

int cz_engine_flush_out(cz_engine *e)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_flush_out: null engine");
    hipError_t he = hipSetDevice(e->device);
    if (he != hipSuccess)
        return hip_fail(he, "hipSetDevice");
    const int rc = e->flush_out();
    if (rc != CZ_OK)
        e->drain();  // an error return may leave copies into/out of the pinned buffers in flight
    return rc;
}

int cz_engine_wire_out(cz_engine *e, int conn, const uint8_t **wire, uint64_t *len)
{
    if (!e || !wire || !len)
        return fail(CZ_EINVAL, "cz_engine_wire_out: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    const uint8_t *base = (const uint8_t *)e->h_wire.ptr;
    if (c->runs.size() <= 1) {  // frames queued together: the stream lies in the flush output as is
        *wire = c->runs.empty() ? base : base + c->runs[0].off;
        *len = c->runs.empty() ? 0 : c->runs[0].len;
        return CZ_OK;
    }
    if (c->gathered.empty()) {  // interleaved with other connections: one host gather
        uint64_t t = 0;
        for (const Run &r : c->runs)
            t += r.len;
        c->gathered.resize(t);
        t = 0;
        for (const Run &r : c->runs) {
            memcpy(c->gathered.data() + t, base + r.off, r.len);
            t += r.len;
        }
    }
    *wire = c->gathered.data();
    *len = c->gathered.size();
    return CZ_OK;
}

int cz_engine_wire_iov(cz_engine *e, int conn, cz_iovec *iov, uint32_t cap, uint32_t *count)
{
    if (!e || !count || (cap && !iov))
        return fail(CZ_EINVAL, "cz_engine_wire_iov: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    *count = (uint32_t)c->runs.size();
    if (cap < c->runs.size())
        return cap ? fail(CZ_EINVAL, "cz_engine_wire_iov: %u pieces, capacity %u", *count, cap) : CZ_OK;
    const uint8_t *base = (const uint8_t *)e->h_wire.ptr;
    for (size_t k = 0; k < c->runs.size(); k++)
        iov[k] = {base + c->runs[k].off, c->runs[k].len};
    return CZ_OK;
}

int cz_engine_recv(cz_engine *e, int conn, const void *wire, uint64_t len)
{
    if (!e || (len && !wire))
        return fail(CZ_EINVAL, "cz_engine_recv: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (c->error)
        return fail(c->error, "cz_engine_recv: connection %d has failed", conn);
    hipError_t he = e->rxpool.grow(c->rx, c->rx_len, c->rx_len + len);
    if (he != hipSuccess)
        return hip_fail(he, "cz_engine_recv: hipHostMalloc");
    if (len)
        memcpy((uint8_t *)c->rx.ptr + c->rx_len, wire, len);
    c->rx_len += len;
    return CZ_OK;
}

int cz_engine_recv_buffer(cz_engine *e, int conn, uint64_t min_bytes, uint8_t **buf, uint64_t *avail)
{
    if (!e || !buf || !avail)
        return fail(CZ_EINVAL, "cz_engine_recv_buffer: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (c->error)
        return fail(c->error, "cz_engine_recv_buffer: connection %d has failed", conn);
    hipError_t he = e->rxpool.grow(c->rx, c->rx_len, c->rx_len + std::max<uint64_t>(min_bytes, 1));
    if (he != hipSuccess)
        return hip_fail(he, "cz_engine_recv_buffer: hipHostMalloc");
    *buf = (uint8_t *)c->rx.ptr + c->rx_len;
    *avail = c->rx.cap - c->rx_len;
    return CZ_OK;
}

int cz_engine_recv_commit(cz_engine *e, int conn, uint64_t n)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_recv_commit: null engine");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (n > c->rx.cap - c->rx_len)
        return fail(CZ_EINVAL, "cz_engine_recv_commit: %llu bytes exceed the buffer", (unsigned long long)n);
    c->rx_len += n;
    return CZ_OK;
}

int cz_engine_flush_in(cz_engine *e)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_flush_in: null engine");
    hipError_t he = hipSetDevice(e->device);
    if (he != hipSuccess)
        return hip_fail(he, "hipSetDevice");
    const int rc = e->flush_in();
    if (rc != CZ_OK)
        e->drain();  // an error return may leave copies into/out of the pinned buffers in flight
    return rc;
}

int cz_engine_forward(cz_engine *e, int from, int to)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_forward: null engine");
    const auto live = [e](int id) { return id >= 0 && (size_t)id < e->conns.size() && !e->conns[(size_t)id].removed; };
    if (!e->routes.set(from, to, live))
        return fail(CZ_EINVAL,
                    "cz_engine_forward: %d -> %d: an unknown connection, from == to, or a destination that has a source",
                    from, to);
    return CZ_OK;
}

int cz_engine_flush_forward(cz_engine *e)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_flush_forward: null engine");
    hipError_t he = hipSetDevice(e->device);
    if (he != hipSuccess)
        return hip_fail(he, "hipSetDevice");
    const int rc = e->flush_forward();
    if (rc != CZ_OK)
        e->drain();  // an error return may leave copies into/out of the pinned buffers in flight
    return rc;
}

int cz_engine_forward_out(cz_engine *e, int from, const uint8_t **wire, uint64_t *len)
{
    if (!e || !wire || !len)
        return fail(CZ_EINVAL, "cz_engine_forward_out: null pointer");
    Conn *c = e->conn(from);
    if (!c)
        return CZ_EINVAL;
    *wire = (const uint8_t *)e->h_fwd.ptr + c->fwd_off;
    *len = c->fwd_len;
    return CZ_OK;
}

int cz_engine_msgs_in(cz_engine *e, int conn, uint32_t *count)
{
    if (!e || !count)
        return fail(CZ_EINVAL, "cz_engine_msgs_in: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    *count = (uint32_t)c->in_msgs.size();
    return CZ_OK;
}

int cz_engine_msg_in(cz_engine *e, int conn, uint32_t i, const uint8_t **payload, uint32_t *len, int *msg_flags)
{
    if (!e || !payload || !len || !msg_flags)
        return fail(CZ_EINVAL, "cz_engine_msg_in: null pointer");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (i >= c->in_msgs.size())
        return fail(CZ_EINVAL, "cz_engine_msg_in: index %u out of range", i);
    const InMsg &m = e->in_msgs[c->in_msgs[i]];
    *payload = (const uint8_t *)e->h_plain.ptr + m.plain_off;
    *len = m.len;
    *msg_flags = m.flags;
    return CZ_OK;
}

int cz_engine_conn_error(cz_engine *e, int conn, int *event)
{
    if (!e)
        return fail(CZ_EINVAL, "cz_engine_conn_error: null engine");
    Conn *c = e->conn(conn);
    if (!c)
        return CZ_EINVAL;
    if (event)
        *event = c->event;
    return c->error;
}

uint64_t cz_engine_nonce(cz_engine *e, int conn)
{
    Conn *c = e ? e->conn(conn) : nullptr;
    return c ? c->nonce : 0;
}

uint64_t cz_engine_peer_nonce(cz_engine *e, int conn)
{
    Conn *c = e ? e->conn(conn) : nullptr;
    return c ? c->peer_nonce : 0;
}

uint64_t cz_engine_fanin_frames(const cz_engine *e) { return e ? e->fanin_frames : 0; }
uint64_t cz_engine_scan_frames(const cz_engine *e) { return e ? e->scan_frames : 0; }
uint64_t cz_engine_fanin_split_frames(const cz_engine *e) { return e ? e->fanin_split_frames : 0; }
uint64_t cz_engine_forward_frames(const cz_engine *e) { return e ? e->forward_frames : 0; }

}  // extern "C"
