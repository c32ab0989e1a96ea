// cz_launch.h -- the launchers cz_kernels.hip defines, declared once.  cz_kernels.hip includes this
// header too, so a definition that drifts from its declaration does not compile.  No allocation, no
// synchronisation in any of them: safe to capture in a hipGraph.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/curvezmq_mi355x.h"
#include "cz_session.h"

extern "C" {
// uniform batches: frame i at in + i * in_stride, output i at out + i * out_stride (cz_dispatch.h picks the kernel)
hipError_t czk_seal_uniform(const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint32_t count,
                            uint32_t len, const void *subkey, uint64_t counter0, const uint8_t *flags8, hipStream_t s);
hipError_t czk_seal_uniform_box(const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint32_t count,
                                uint32_t len, const void *subkey, uint64_t counter0, hipStream_t s);
hipError_t czk_open_uniform(const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint32_t count,
                            uint32_t size, const void *subkey, uint64_t floor0, int check, uint16_t *status,
                            hipStream_t s);
// 1 when a uniform batch with this out_stride owns its whole slots (the host-staged paths zero the
// slots themselves when it does not).  Host code, no device call.
int czk_owns_slots(uint64_t out_stride);

// PUB fan-out: `count` seals of one payload; a flush group's runs in at most three launches
hipError_t czk_seal_fanout(const void *payload, uint32_t len, uint32_t flags, const cz_fanout_sub *subs,
                           const void *subkeys, void *out, uint64_t out_stride, uint32_t count, hipStream_t s);
hipError_t czk_seal_fanout_runs(const cz_fanout_run *runs, const cz_fanout_wave *waves, const uint32_t class_count[3],
                                uint32_t region_stride, const void *in, const cz_fanout_sub *subs,
                                const void *subkeys, void *out, hipStream_t s);
// The staging class cz_plan_fanout gives the full waves of a run (CZ_FANOUT_LINES / _REGION /
// _DIRECT): czk_seal_fanout's choice for that run alone.  Host code, no device call.
int czk_fanout_class(uint64_t out_stride, uint32_t len, uint32_t count, int aligned);
// split PUB fan-out: lanes are (run, subscriber, segment); tiles by class, then the join
hipError_t czk_seal_fanout_split(const cz_fanout_run *runs, const cz_fanout_tile *tiles, const uint32_t class_count[2],
                                 const cz_fanout_join *joins, uint32_t njoins, const void *in,
                                 const cz_fanout_sub *subs, const void *subkeys, void *out, void *work, hipStream_t s);

// fan-in open: runs of same-size bodies of many connections, one lane per body, at most three launches
hipError_t czk_open_fanin_runs(const cz_fanin_run *runs, const cz_fanout_wave *waves, const uint32_t class_count[3],
                               uint32_t region_stride, const void *in, const cz_fanin_sub *subs, const void *subkeys,
                               void *out, uint16_t *status, uint64_t *nonces, hipStream_t s);
// The staging class cz_plan_fanin gives the full waves of a run.  Host code, no device call.
int czk_fanin_class(uint64_t out_stride, uint32_t size, uint32_t count, int aligned);
// split fan-in open: lanes are (run, body, segment); tiles by class, then the join
hipError_t czk_open_fanin_split(const cz_fanin_run *runs, const cz_fanout_tile *tiles, const uint32_t class_count[2],
                                const cz_fanout_join *joins, uint32_t njoins, const void *in,
                                const cz_fanin_sub *subs, const void *subkeys, void *out, void *work,
                                uint16_t *status, uint64_t *nonces, hipStream_t s);

// descriptor and segmented (ragged) batches
hipError_t czk_seal_desc(const cz_frame_desc *desc, const uint32_t *order, uint32_t count, const void *in, void *out,
                         const void *subkeys, hipStream_t s);
hipError_t czk_open_desc(const cz_frame_desc *desc, const uint32_t *order, uint32_t count, const void *in, void *out,
                         const void *subkeys, uint16_t *status, uint64_t *nonces, hipStream_t s);
hipError_t czk_seal_segments(const cz_frame_desc *desc, const cz_segment *segs, uint32_t nseg, const cz_combine *comb,
                             uint32_t ncomb, const void *in, void *out, const void *subkeys, void *work, hipStream_t s);
hipError_t czk_open_segments(const cz_frame_desc *desc, const cz_segment *segs, uint32_t nseg, const cz_combine *comb,
                             uint32_t ncomb, const void *in, void *out, const void *subkeys, void *work,
                             uint16_t *status, uint64_t *nonces, hipStream_t s);
hipError_t czk_v2_copy(const cz_v2_item *items, uint32_t count, const void *src, void *dst, hipStream_t s);
// device V2 scan: one lane per stream walks its headers (k_v2_scan), one workgroup places the streams
// (k_v2_place: first / slot_off, the totals record); then the same walk writes frames and / or descriptors
hipError_t czk_v2_scan(const cz_v2_stream *streams, uint32_t count, const void *wire, int64_t maxmsgsize,
                       uint32_t slot_align, cz_v2_stream_result *results, cz_v2_totals *totals, hipStream_t s);
hipError_t czk_v2_emit(const cz_v2_stream *streams, const cz_v2_stream_result *results, uint32_t count,
                       const void *wire, uint32_t slot_align, cz_v2_frame *frames, cz_frame_desc *desc, hipStream_t s);
// stream relay: the walk once more writes the relay's descriptors (materialised floors, no prev, bodies where
// they lie) and per-frame outbound records, and the headers when out != wire (k_v2_emit_relay); behind
// czk_relay_desc, one lane per stream cuts its stream at the first rejected frame (k_relay_cut)
hipError_t czk_v2_emit_relay(const cz_v2_stream *streams, const cz_fanout_sub *to, const cz_v2_stream_result *results,
                             uint32_t count, const void *wire, void *out, cz_frame_desc *desc, cz_fanout_sub *to_frames,
                             hipStream_t s);
hipError_t czk_relay_cut(const cz_v2_stream *streams, const cz_v2_stream_result *results, uint32_t count,
                         const cz_frame_desc *desc, const uint16_t *status, const uint64_t *nonces,
                         cz_relay_stream_result *cut, hipStream_t s);

// CURVE relay: received bodies re-sealed for another peer in one pass (descriptor batch; one connection to one)
hipError_t czk_relay_desc(const cz_frame_desc *desc, const cz_fanout_sub *to, const uint32_t *order, uint32_t count,
                          const void *in, void *out, const void *subkeys, uint16_t *status, uint64_t *nonces,
                          hipStream_t s);
hipError_t czk_relay_uniform(const void *in, uint64_t in_stride, void *out, uint64_t out_stride, uint32_t count,
                             uint32_t size, const void *subkey_in, uint64_t floor0, int check, const void *subkey_out,
                             uint64_t counter0, uint16_t *status, hipStream_t s);
// segmented relay: one lane per segment (two planes of npart 64-byte records in `work`), then the combine
hipError_t czk_relay_segments(const cz_frame_desc *desc, const cz_fanout_sub *to, const cz_segment *segs, uint32_t nseg,
                              const cz_combine *comb, uint32_t ncomb, uint32_t npart, const void *in, void *out,
                              const void *subkeys, void *work, uint16_t *status, uint64_t *nonces, hipStream_t s);

// one NaCl box in one launch
hipError_t czk_nacl_one(void *st, uint32_t len, int open, void *subcache, int miss, uint32_t out_off,
                        const uint8_t k[32], const uint8_t n[24], hipStream_t s);
uint32_t czk_nacl_one_max(void);    // one pass of k_nacl_one: the size up to which one launch beats the segment kernels
uint32_t czk_nacl_one_limit(void);  // the largest box k_nacl_one takes

// subkeys
hipError_t czk_subkeys(const void *precom, void *out, uint32_t nkeys, const uint8_t prefix[16], hipStream_t s);
// table[32 * tx_key], table[32 * rx_key] = HSalsa20(cnPrecom, MESSAGE prefix) for jobs[0, count)
hipError_t czk_session_subkeys(const cz_session_job *d_jobs, uint32_t count, const void *d_base, void *d_table,
                               hipStream_t s);
// zero rec_bytes (a multiple of 16) at base + offset + idx[i] * rec_bytes for i in [0, count); base + offset
// 16-byte aligned
hipError_t czk_scatter_wipe(void *d_base, const uint32_t *d_idx, uint32_t count, uint32_t rec_bytes, uint64_t offset,
                            hipStream_t s);

hipError_t czk_copy16(void *dst, const void *src, uint64_t nbytes, hipStream_t s);
hipError_t czk_fill(void *buf, uint64_t nbytes, uint64_t seed, hipStream_t s);

// run-time knobs (czd::Knobs): the old value, or -1 for an unknown key
int czk_tune(const char *key, int value);
}
