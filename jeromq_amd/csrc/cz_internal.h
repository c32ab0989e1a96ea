// cz_internal.h -- shared host-side helpers of libcurvezmq_mi355x (not part of the C-ABI).  The handshake's
// parsers are in cz_hs_parse.h, what the batched acceptor and connector share in cz_hs_batch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/curvezmq_mi355x.h"
#include "cz_hs_parse.h"
#include "cz_launch.h"

namespace czi {

int fail(int code, const char *fmt, ...);
int hs_thread_init();  // the calling thread's handshake context (cz_handshake.cpp)
uint64_t nacl_one_bytes();  // boxes up to this size take k_nacl_one (cz_tune "nacl_one_max")
uint32_t fanout_min();      // publish runs of at least this many frames take k_seal_fanout (cz_tune "fanout_min")
uint32_t fanout_short();    // ... and runs of a full wave or more with payloads up to this (cz_tune "fanout_short")
int hip_fail(hipError_t e, const char *where);
const uint8_t *prefix_for(int direction);
void plan_segments(const cz_frame_desc *h_desc, uint32_t count, int open, uint32_t seg_blocks,
                   std::vector<cz_segment> &segs, std::vector<cz_combine> &combs, uint32_t &npart);

// The wave table of a grouped fan-out (cz_plan_fanout) for runs already validated: waves[0, nwaves) sorted by
// class (CZ_FANOUT_LINES, _REGION, _DIRECT), longest payload first inside a class; returns the largest region stride.
// `waves` must hold fanout_waves(runs, nruns) records.
uint64_t fanout_waves(const cz_fanout_run *runs, uint32_t nruns);
uint32_t plan_fanout(const cz_fanout_run *runs, uint32_t nruns, const void *d_in, const void *d_out, cz_fanout_wave *waves,
                     uint32_t class_count[3]);

// The wave table of a fan-in open (cz_plan_fanin) for runs already validated, as plan_fanout: sorted by class,
// longest body first inside a class; returns the largest region stride.  `waves` must hold fanin_waves(...) records.
uint32_t fanin_short();  // received runs of a full wave or more with payloads up to this take cz_open_fanin_runs (cz_tune "fanin_short")
uint64_t fanin_waves(const cz_fanin_run *runs, uint32_t nruns);
uint32_t plan_fanin(const cz_fanin_run *runs, uint32_t nruns, const void *d_in, const void *d_out, cz_fanout_wave *waves,
                    uint32_t class_count[3]);

// The tables of a split fan-out (cz_plan_fanout_split) for runs already validated and seg_blocks >= 1:
// `tiles` / `joins` must hold fanout_split_counts(...).ntiles / .njoins records.
struct FanoutSplitCounts {
    uint64_t ntiles, njoins, npart;
};
uint32_t fanout_split();  // publish runs of a full wave or more with payloads of at least this take the split fan-out (cz_tune "fanout_split")
uint32_t fanout_split_seg_blocks(const cz_fanout_run *runs, uint32_t nruns);  // seg_blocks == 0
FanoutSplitCounts fanout_split_counts(const cz_fanout_run *runs, uint32_t nruns, uint32_t seg_blocks);
void plan_fanout_split(const cz_fanout_run *runs, uint32_t nruns, const void *d_in, uint32_t seg_blocks,
                       cz_fanout_tile *tiles, uint32_t class_count[2], cz_fanout_join *joins);

// The tables of a split fan-in open (cz_plan_fanin_split) for runs already validated and seg_blocks >= 1:
// `tiles` / `joins` must hold fanin_split_counts(...).ntiles / .njoins records.
uint32_t fanin_split();  // received runs of a full wave or more with payloads of at least this take the split fan-in (cz_tune "fanin_split")
uint32_t fanin_split_seg_blocks(const cz_fanin_run *runs, uint32_t nruns);  // seg_blocks == 0
FanoutSplitCounts fanin_split_counts(const cz_fanin_run *runs, uint32_t nruns, uint32_t seg_blocks);
void plan_fanin_split(const cz_fanin_run *runs, uint32_t nruns, const void *d_in, uint32_t seg_blocks,
                      cz_fanout_tile *tiles, uint32_t class_count[2], cz_fanout_join *joins);

uint32_t scan_in();  // a flush of at least 64 receiving connections with at most this many bytes each is parsed on the device (cz_tune "scan_in")

// Segment length for a received flush of `blocks` 64-byte blocks in all (cz_engine_flush_in learns its
// frame sizes only from the parse): SEG_BLOCKS (128, the throughput setting) once
// there are 64K lanes' worth, shorter below that (down to 4) so that a small flush spreads each frame
// over many lanes instead of walking it on one (a 4 KiB frame alone: 65 blocks on one lane, ~150 us).
// flush_out knows its lengths up front and uses batch_seg_blocks.
inline uint32_t flush_seg_blocks(uint64_t blocks)
{
    const uint64_t s = (blocks + 65535) / 65536;
    return (uint32_t)(s < 4 ? 4 : s > 128 ? 128 : s);
}

// segments, combine records and partial records the planner makes for one frame of `len` (payload for seal, body
// for open) -- lets a caller size its buffers before planning
inline void plan_counts(uint64_t len, int open, uint32_t seg_blocks, uint64_t &nseg, uint64_t &ncomb, uint64_t &npart)
{
    const uint64_t mlen = open ? len : len + CZ_MESSAGE_OVERHEAD;
    uint64_t nblk = (mlen + 63) / 64;
    if (nblk == 0)
        nblk = 1;
    if (nblk <= seg_blocks + seg_blocks / 2) {
        nseg += 1;
        return;
    }
    const uint64_t lead = open ? 1u : 0u;
    const uint64_t ns = (nblk - lead + seg_blocks - 1) / seg_blocks;
    nseg += ns;
    npart += ns;
    ncomb += 1;
}

// Segment length for ONE frame of nblk blocks on its own: a lane walks seg + 1 blocks (block 0
// gives its Poly1305 key) and the combine lane walks the nblk / seg segments serially, so the
// latency is ~ (seg + 1) * T_block + (nblk / seg) * T_combine, T_block / T_combine ~ 18
// (DESIGN.md section 4).
inline uint32_t single_seg_blocks(uint64_t nblk)
{
    uint32_t s = 2;
    while ((uint64_t)(s + 1) * (s + 1) * 18 <= nblk)
        s++;
    return s;
}

// Segment length for a batch of `total` blocks whose longest frame has `longest` blocks: 128
// (SEG_BLOCKS, the throughput setting) once the batch has 64K lanes' worth, shorter below that, so
// a small batch spreads its frames over many lanes; never shorter than the one-frame optimum.
inline uint32_t batch_seg_blocks(uint64_t total, uint64_t longest)
{
    uint64_t s = (total + 65535) / 65536;
    s = s > single_seg_blocks(longest) ? s : single_seg_blocks(longest);
    return (uint32_t)(s < 128 ? s : 128);
}

// device buffer that grows on demand (never shrinks)
struct DevBuf {
    void *ptr = nullptr;
    uint64_t cap = 0;
    hipError_t reserve(uint64_t bytes);
    void release();
};

// pinned host buffer that grows on demand
struct HostBuf {
    void *ptr = nullptr;
    uint64_t cap = 0;
    hipError_t reserve(uint64_t bytes);
    void release();
};

// (the handshake parsers shared by cz_hs, cz_acceptor and cz_connector: cz_hs_parse.h)
void secure_wipe(void *p, size_t n);
void secure_wipe(std::vector<uint8_t> &v);

}  // namespace czi
