// cz_dispatch.h -- which kernel a batch gets: the launchers' decisions as pure functions.
//
// Host arithmetic only: no HIP call, no global.  Every plan_* function maps a layout (addresses,
// strides, count, length) and the run-time knobs to the instantiation, the grid, the dynamic LDS
// bytes and the zero-pad launch of one launcher of cz_kernels.hip, which launches what the plan
// says and decides nothing itself.  The launch geometry and the stride and size limits the kernels
// share with these decisions are defined here, once.  Not part of the C-ABI.
#pragma once
#include <stdint.h>

#include "../../include/curvezmq_mi355x.h"

#if defined(__HIP__)  // (the kernels use owns_slots too)
#define CZD_HD __host__ __device__ __forceinline__
#else
#define CZD_HD inline
#endif

namespace czd {

// MODE_BOX: MESSAGE output (as MODE_ZMQ) from input already in the reference's box layout,
// m = 0^32 || flags || payload (CurveClientMechanism.java:144-153 builds exactly this and hands it
// to Curve.afternm): box blocks are read where they lie, no funnel shift, no carried words.
enum Mode { MODE_ZMQ = 0, MODE_NACL = 1, MODE_BOX = 2 };
// the emitter of a uniform kernel (cz_kernels.hip's header): EmitDirect, EmitLines, EmitRegion,
// EmitShiftLinesUni
enum Staging { ST_DIRECT = 0, ST_LINES = 1, ST_REGION = 2, ST_SHIFT = 3 };

constexpr int BLOCK = 256;  // threads per workgroup (4 waves)
constexpr int WAVES = BLOCK / 64;
constexpr uint32_t LINE_LDS_BYTES = 64 * 128;  // EmitLines: one 128-byte line per frame
constexpr uint32_t HOLD_LDS_BYTES = 64 * 64;   // EmitLines (seal): block 1 of every frame, until tag()
constexpr uint32_t SROW = 208;  // 16 headroom + 192 bytes used; 52 dwords apart: conflict-free 16-lane b128
constexpr uint32_t SHIFT_LDS_BYTES = 64 * SROW;  // EmitShiftLines: 13 KiB per wave
// the uniform seal's rows (EmitShiftLinesT WHOLE) + 16 bytes: the next body's header, written behind
// an output's end at row byte <= 192, may run 16 bytes past the last row
constexpr uint32_t SEAL_SHIFT_LDS_BYTES = WAVES * SHIFT_LDS_BYTES + 16u;

// ---- limits -----------------------------------------------------------------
constexpr uint32_t REGION_MAX = 16384;  // EmitRegion: 64 slots per wave
// EmitLines' buffer-store offsets, up to 64 * stride, stay below 2^31 (and a larger slot is not
// worth zeroing)
constexpr uint64_t LINES_STRIDE_MAX = 1ull << 25;
// EmitShiftLinesUni's buffer-store offsets, below 256 * stride + len + 160, stay below 2^31
constexpr uint64_t SHIFT_STRIDE_MAX = 1ull << 22;
// the line emitters take bodies of at least two lines
constexpr uint32_t LINES_BYTES_MIN = 256;
// EmitShiftLinesT keeps its flag bits 28..31 (tag_whole, ext_end, ext_start, tag slot) above the
// output's end d + total in `te`, so an output goes to ST_SHIFT only when d + total < 2^28 with
// d < 128: total <= SHIFT_TOTAL_MAX.
constexpr uint32_t SHIFT_TE_FLAG_BITS = 0xf0000000u;
constexpr uint32_t SHIFT_TOTAL_MAX = (1u << 28) - 128u;
static_assert(((SHIFT_TOTAL_MAX + 127u) & SHIFT_TE_FLAG_BITS) == 0u, "te's end field overlaps its flag bits");

// ---- segment kernels' mode word ---------------------------------------------
constexpr int SEGMODE_LINES = 1;    // line-staged stores for waves of equal-length segments
constexpr int SEGMODE_PAIR = 2;     // whole-line input loads (seal)
constexpr int SEGMODE_REST = 4;     // k_seal_segments: only the waves k_seal_segments_lines leaves
constexpr int SEGMODE_SHIFT16 = 8;  // 16-byte aligned outputs not all on 128-byte lines: EmitShiftLines
constexpr int SEGMODE_ANYIN = 16;   // inputs at any byte offset on the line paths (dword-aligned loads)

// ---- run-time knobs (cz_tune) -------------------------------------------------
#ifndef CZ_OPEN_CARRY_DEFAULT
#define CZ_OPEN_CARRY_DEFAULT 1
#endif
#ifndef CZ_SHIFT16_DEFAULT
#define CZ_SHIFT16_DEFAULT 1
#endif
struct Knobs {
    int pair = 1;      // whole-line input loads for the uniform kernels
    int un0 = 1;       // scalar first Salsa round when the high nonce word is wave-uniform
    int seglines = 1;  // line-staged stores for waves of equal-length segments
    int shift = 1;     // uniform seal / open: shifted line staging for bodies at any byte offset
    int open_ina = 1;  // uniform open: line path for bodies off 16-byte alignment (dword-aligned loads)
    int seal_ina = 1;  // seal: staged / line paths for payloads off 16-byte alignment
    // uniform open off 16-byte alignment: phase-sorted waves, carried lines (2: INA 1 too, A/B only)
    int open_carry = CZ_OPEN_CARRY_DEFAULT;
    // segment kernels: waves of 16-byte aligned outputs that are not all on 128-byte lines go through
    // EmitShiftLines (whole cache lines) instead of EmitSegLines (128-byte groups at each output's
    // base, two partial cache lines per group): Zipf seal with 16-byte output slots 1250 -> 1629 GiB/s
    int shift16 = CZ_SHIFT16_DEFAULT;
};

// ---- what a launcher launches -----------------------------------------------
enum Family { K_SEAL_UNIFORM, K_SEAL_UNIFORM_INA, K_SEAL_FANOUT, K_OPEN_UNIFORM, K_OPEN_UNIFORM_CARRY, K_SEAL_FANOUT_TILES, K_OPEN_FANIN, K_OPEN_FANIN_TILES, K_RELAY_UNIFORM };
constexpr int64_t PAD_NONE = -1;

struct Launch {
    int family;  // Family
    int st;      // Staging
    bool pair;   // whole-line input loads
    int ina;     // input alignment the loads may assume: 16, 8 or 1
    int mode;    // Mode
    uint32_t grid;
    uint32_t lds;      // dynamic LDS bytes
    int64_t pad_from;  // k_zero_pad zeroes bytes [pad_from, stride) of every slot; PAD_NONE: no such launch
};

// czk_open_uniform: `head` alone (done = 0), or for the carried open `head` = k_open_uniform_carry
// over the first `done` frames (nwaves waves, line phase period P) and, if frames are left, `tail` =
// k_open_uniform over the rest
struct OpenLaunch {
    Launch head, tail;
    uint32_t P, nwaves;
    uint64_t done;
};

// czk_relay_uniform: `head` over the first `done` frames and, when done < count, the lane-wise `tail`
// over the frames behind the last full wave
struct RelayLaunch {
    Launch head, tail;
    uint32_t done;
};

// The output-ownership rule of a uniform batch and of a fan-out run (header sections 3 and 3c), by
// the stride alone: whichever emitter the alignments and the length select, the slots of such a
// batch are written whole.
CZD_HD bool owns_slots(uint64_t out_stride)
{
    return (out_stride % 128 == 0 && out_stride < LINES_STRIDE_MAX) || (out_stride % 16 == 0 && 64 * out_stride <= REGION_MAX);
}

inline bool aligned16(uint64_t bits) { return (bits & 15u) == 0; }
inline int input_alignment(uint64_t bits) { return (bits & 15u) == 0 ? 16 : (bits & 7u) == 0 ? 8 : 1; }
inline uint32_t blocks_for(uint32_t lanes) { return (lanes + BLOCK - 1) / BLOCK; }

// Staging choice for a uniform batch whose pointers and strides are all 16-byte aligned (`aligned`).
inline int pick_staging(uint64_t stride, uint32_t out_bytes, bool aligned)
{
    if (!aligned)
        return ST_DIRECT;
    if (stride % 128 == 0 && out_bytes >= LINES_BYTES_MIN && stride < LINES_STRIDE_MAX)
        return ST_LINES;
    if (stride % 16 == 0 && 64 * stride <= REGION_MAX)
        return ST_REGION;
    return ST_DIRECT;
}

// ... and for outputs at any byte offset (dense slots, the wire layout): shifted line staging where
// pick_staging leaves lane-wise stores
inline int pick_staging_shift(uint64_t stride, uint32_t out_bytes, bool aligned, const Knobs &k)
{
    const int st = pick_staging(stride, out_bytes, aligned);
    if (st == ST_DIRECT && out_bytes >= LINES_BYTES_MIN && out_bytes <= SHIFT_TOTAL_MAX && stride < SHIFT_STRIDE_MAX && k.shift)
        return ST_SHIFT;
    return st;
}

inline uint32_t staging_lds(int st, uint64_t out_stride, bool seal)
{
    switch (st) {
    case ST_LINES: return WAVES * (LINE_LDS_BYTES + (seal ? HOLD_LDS_BYTES : 0u));
    case ST_SHIFT: return seal ? SEAL_SHIFT_LDS_BYTES : WAVES * SHIFT_LDS_BYTES;
    case ST_REGION: return (uint32_t)(WAVES * 64 * out_stride);
    default: return 0u;
    }
}

// The rest of owned slots (header section 3) after a kernel that wrote `bytes` of every slot:
// nothing for the region emitter, which writes whole slots; the line emitter writes to the end of
// the body's last line; nothing where the slot ends there or the batch does not own its slots.
inline int64_t pad_from(int st, uint64_t out_stride, uint32_t bytes)
{
    const uint32_t done = st == ST_LINES ? (bytes + 127u) & ~127u : bytes;
    return st == ST_REGION || out_stride <= done || !owns_slots(out_stride) ? PAD_NONE : (int64_t)done;
}
inline uint32_t pad_grid(uint64_t out_stride, uint32_t count, int64_t from)
{
    const uint64_t total = ((out_stride - (uint64_t)from + 4095u) / 4096u) * count;
    return (uint32_t)(total < (1u << 18) ? total : (1u << 18));
}

inline Launch uniform_launch(int family, int st, bool pair, int ina, int mode, uint32_t count, uint64_t out_stride,
                             uint32_t bytes, bool seal)
{
    return Launch{family, st, pair, ina, mode, blocks_for(count), staging_lds(st, out_stride, seal), pad_from(st, out_stride, bytes)};
}

// czk_seal_uniform: `count` payloads of `len` bytes at in + i * in_stride to MESSAGE bodies at out + i * out_stride
inline Launch plan_seal_uniform(uint64_t in, uint64_t in_stride, uint64_t out, uint64_t out_stride, uint32_t count,
                                uint32_t len, const Knobs &k)
{
    const uint32_t body = len + 33u;
    const bool in_al = aligned16(in | in_stride), out_al = aligned16(out | out_stride);
    // payloads off 16-byte alignment (messages packed back to back): the staged kernels with
    // dword-aligned loads (INA 8 / 1) instead of lane-wise unaligned loads and byte-exact stores
    if (!in_al && k.pair && k.seal_ina && len >= 64u) {
        const int so = pick_staging_shift(out_stride, body, out_al, k);
        if (so != ST_DIRECT)
            return uniform_launch(K_SEAL_UNIFORM_INA, so, so != ST_REGION, input_alignment(in | in_stride) == 8 ? 8 : 1,
                                  MODE_ZMQ, count, out_stride, body, true);
    }
    // bodies at any byte offset take the shifted line staging from aligned payloads only
    const int st = in_al ? pick_staging_shift(out_stride, body, out_al, k) : (int)ST_DIRECT;
    // whole-line input pays for large frames (A/B: 4 KiB seal 2.34 vs 2.51 ms) but
    // not for the small frames of the region stager (100 B: 0.119 vs 0.114 ms)
    return uniform_launch(K_SEAL_UNIFORM, st, k.pair && st != ST_REGION, 16, MODE_ZMQ, count, out_stride, body, true);
}

// czk_seal_uniform_box, box-layout input (MODE_BOX): whole-line staging for 128-byte multiple output
// slots, direct stores otherwise; whole-line input loads always (the box is read where it lies).
inline Launch plan_seal_box(uint64_t in, uint64_t in_stride, uint64_t out, uint64_t out_stride, uint32_t count,
                            uint32_t len, const Knobs &)
{
    const int st = pick_staging(out_stride, len + 33u, aligned16(in | in_stride | out | out_stride));
    return uniform_launch(K_SEAL_UNIFORM, st == ST_LINES ? ST_LINES : ST_DIRECT, true, 16, MODE_BOX, count, out_stride,
                          len + 33u, true);
}

// czk_seal_fanout, and one run of czk_seal_fanout_runs on its own: `count` seals of one payload.
// `aligned`: payload, output base and out_stride all on 16 bytes.  Only full waves are staged; the
// kernel writes the zeros past a body itself (no zero-pad launch).  Whole-line input loads as
// plan_seal_uniform: not for the small frames of the region stager.
inline Launch plan_fanout(uint64_t out_stride, uint32_t len, uint32_t count, bool aligned)
{
    const int st = count >= 64u ? pick_staging(out_stride, len + 33u, aligned) : (int)ST_DIRECT;
    return Launch{K_SEAL_FANOUT, st, st != ST_REGION, 16, MODE_ZMQ, blocks_for(count), staging_lds(st, out_stride, true), PAD_NONE};
}

// the staging class of that run in cz_plan_fanout's wave table
inline int plan_fanout_class(uint64_t out_stride, uint32_t len, uint32_t count, bool aligned)
{
    const int st = plan_fanout(out_stride, len, count, aligned).st;
    return st == ST_LINES ? CZ_FANOUT_LINES : st == ST_REGION ? CZ_FANOUT_REGION : CZ_FANOUT_DIRECT;
}

// czk_seal_fanout_runs: every wave of the region launch gets an LDS partition of 64 slots of the
// largest region stride (0 or above REGION_MAX / 64: REGION_MAX / 64), in 16-byte units
inline uint32_t fanout_region_part16(uint32_t region_stride)
{
    const uint32_t rs = region_stride == 0 || region_stride > REGION_MAX / 64 ? REGION_MAX / 64 : region_stride;
    return (64u * ((rs + 15u) & ~15u)) >> 4;
}
// ... and the launch of one class's slice of the wave table (`nwaves` waves, one per 64 lanes)
inline Launch plan_fanout_runs(int cls, uint32_t nwaves, uint32_t part16)
{
    const int st = cls == CZ_FANOUT_LINES ? ST_LINES : (cls == CZ_FANOUT_REGION ? ST_REGION : ST_DIRECT);
    return Launch{K_SEAL_FANOUT, st, st != ST_REGION, 16, MODE_ZMQ, (nwaves + WAVES - 1) / WAVES,
                  st == ST_REGION ? (uint32_t)(WAVES * 16u * part16) : staging_lds(st, 0, true), PAD_NONE};
}

// czk_open_fanin_runs: the staging class of a run's full waves in cz_plan_fanin's wave table -- what
// pick_staging gives its plaintext slots when body base, in_stride, output base and out_stride are all
// on 16 bytes (`aligned`); a run without a full wave is lane-wise
inline int plan_fanin_class(uint64_t out_stride, uint32_t size, uint32_t count, bool aligned)
{
    const int st = count >= 64u ? pick_staging(out_stride, size >= 33u ? size - 33u : 0u, aligned) : (int)ST_DIRECT;
    return st == ST_LINES ? CZ_FANOUT_LINES : st == ST_REGION ? CZ_FANOUT_REGION : CZ_FANOUT_DIRECT;
}
// ... and the launch of one class's slice of the wave table (`nwaves` waves, one per 64 lanes): the
// emitters and whole-line loads of k_open_uniform's same class, the region partition of plan_fanout_runs
inline Launch plan_fanin_runs(int cls, uint32_t nwaves, uint32_t part16)
{
    const int st = cls == CZ_FANOUT_LINES ? ST_LINES : (cls == CZ_FANOUT_REGION ? ST_REGION : ST_DIRECT);
    return Launch{K_OPEN_FANIN, st, st != ST_REGION, 16, MODE_ZMQ, (nwaves + WAVES - 1) / WAVES,
                  st == ST_REGION ? (uint32_t)(WAVES * 16u * part16) : staging_lds(st, 0, false), PAD_NONE};
}

// czk_seal_fanout_split: one class's slice of the tile table, one wave per tile; the line class stages
// through the segment emitters' rows (EmitSegLines / EmitShiftLines), the lane-wise class needs no LDS
inline Launch plan_fanout_tiles(int cls, uint32_t ntiles)
{
    const int st = cls == CZ_FANOUT_TILE_LINES ? ST_LINES : ST_DIRECT;
    return Launch{K_SEAL_FANOUT_TILES, st, true, 16, MODE_ZMQ, (ntiles + WAVES - 1) / WAVES,
                  st == ST_LINES ? WAVES * SHIFT_LDS_BYTES : 0u, PAD_NONE};
}

// czk_open_fanin_split: one class's slice of the tile table, one wave per tile; the line class stages
// through k_open_segments' rows (EmitSegLines / EmitShiftLines), the lane-wise class needs no LDS
inline Launch plan_fanin_tiles(int cls, uint32_t ntiles)
{
    const int st = cls == CZ_FANOUT_TILE_LINES ? ST_LINES : ST_DIRECT;
    return Launch{K_OPEN_FANIN_TILES, st, true, 16, MODE_ZMQ, (ntiles + WAVES - 1) / WAVES,
                  st == ST_LINES ? WAVES * SHIFT_LDS_BYTES : 0u, PAD_NONE};
}

// czk_open_uniform: `count` MESSAGE bodies of `size` bytes at in + i * in_stride to plaintext at out + i * out_stride
inline OpenLaunch plan_open_uniform(uint64_t in, uint64_t in_stride, uint64_t out, uint64_t out_stride, uint32_t count,
                                    uint32_t size, const Knobs &k)
{
    const uint32_t nout = size >= 33u ? size - 33u : 0u;
    const int ina = input_alignment(in | in_stride);
    // bodies off 16-byte alignment (the dense wire layout) into aligned plaintext slots keep the
    // staged emitters, with dword-aligned loads (INA 8 / 1); plaintext at any byte offset (slots
    // that are not 128-byte multiples) takes byte-shifted line staging, as the seal's bodies
    const int st_out = size >= 33u ? pick_staging_shift(out_stride, nout, aligned16(out | out_stride), k) : (int)ST_DIRECT;
    auto launch = [&](int family, int st, bool pair, int ina, uint32_t n) {
        return uniform_launch(family, st, pair, ina, MODE_ZMQ, n, out_stride, nout, false);
    };
    // small bodies (64 plaintext slots <= 16 KiB) off 16-byte alignment: region staging
    if (ina != 16 && st_out == ST_REGION && k.open_ina)
        return OpenLaunch{launch(K_OPEN_UNIFORM, ST_REGION, false, ina, count)};
    // (INA 1 -- any byte offset -- measured 1.3% slower with carried lines at 2 waves per SIMD than
    // the straddling loads at 3, so only 8-byte aligned bodies take it: +2.6%)
    // (cz_tune("open_carry", 2): INA 1 too, A/B only)
    if (k.pair && st_out == ST_LINES && (ina == 8 || (ina == 1 && k.open_carry == 2)) && k.open_ina && k.open_carry &&
        nout >= LINES_BYTES_MIN) {
        // phase-sorted waves with carried aligned lines (k_open_uniform_carry): whole blocks of 64 P
        // frames, P = the period of the bodies' line phase, 128 / gcd(in_stride mod 128, 128) -- the
        // lowest set bit of in_stride up to 128; the rest through k_open_uniform
        const uint64_t low = in_stride | 128u;
        const uint32_t P = 128u / (uint32_t)(low & (0 - low));
        const uint64_t blocks = count / (64ull * P);
        if (blocks > 0 && 64ull * P * out_stride < (1ull << 31)) {
            OpenLaunch p{launch(K_OPEN_UNIFORM_CARRY, ST_LINES, true, ina, count),
                         launch(K_OPEN_UNIFORM, ST_LINES, true, ina, count - (uint32_t)(blocks * 64ull * P)), P,
                         (uint32_t)(blocks * P), blocks * 64ull * P};
            p.head.grid = (p.nwaves + WAVES - 1) / WAVES;
            p.tail.pad_from = PAD_NONE;  // head's covers every slot
            return p;
        }
    }
    if (k.pair && (st_out == ST_SHIFT || (st_out == ST_LINES && ina != 16)) && (ina == 16 || k.open_ina))
        return OpenLaunch{launch(K_OPEN_UNIFORM, st_out, true, ina, count)};
    // everything 16-byte aligned: the staged emitters, whole-line input as the seal; else lane-wise
    const int st = size >= 33u ? pick_staging(out_stride, nout, ina == 16 && aligned16(out | out_stride)) : (int)ST_DIRECT;
    return OpenLaunch{launch(K_OPEN_UNIFORM, st, k.pair && st != ST_REGION, 16, count)};
}

// czk_relay_uniform: `count` MESSAGE bodies of `size` bytes at in + i * in_stride re-sealed to out + i * out_stride.
// The seal's line emitter takes the full waves when body base, in_stride, output base and out_stride are
// all on 16 bytes, out_stride is a line multiple below LINES_STRIDE_MAX and the body has two lines; the
// frames behind the last full wave, and every other layout (the dense stride, short bodies, sizes
// below a MESSAGE's 33 bytes), go lane-wise.  Both kernels write the zeros of owned slots themselves:
// no zero-pad launch.  No knob changes this plan.
inline RelayLaunch plan_relay_uniform(uint64_t in, uint64_t in_stride, uint64_t out, uint64_t out_stride, uint32_t count,
                                      uint32_t size)
{
    auto launch = [&](int st, uint32_t n) {
        return Launch{K_RELAY_UNIFORM, st, false, 16, MODE_ZMQ, blocks_for(n), staging_lds(st, out_stride, true), PAD_NONE};
    };
    const bool lines = aligned16(in | in_stride | out | out_stride) && out_stride % 128 == 0 &&
                       out_stride < LINES_STRIDE_MAX && size >= LINES_BYTES_MIN;
    const uint32_t full = count & ~63u;
    if (lines && full)
        return RelayLaunch{launch(ST_LINES, full), launch(ST_DIRECT, count - full), full};
    return RelayLaunch{launch(ST_DIRECT, count), launch(ST_DIRECT, 0), count};
}

// ---- segment launchers --------------------------------------------------------
// czk_seal_segments: with line staging and whole-line loads both on, k_seal_segments_lines takes the
// full waves of aligned segments and k_seal_segments the rest (SEGMODE_REST, set by the launcher
// on that second launch); otherwise k_seal_segments alone runs every wave.
inline bool seal_segments_two_pass(const Knobs &k) { return k.seglines && k.pair; }
inline int seal_segments_mode(const Knobs &k)
{
    if (seal_segments_two_pass(k))
        return SEGMODE_LINES | SEGMODE_PAIR | (k.shift16 ? SEGMODE_SHIFT16 : 0) | (k.seal_ina ? SEGMODE_ANYIN : 0);
    return (k.seglines ? SEGMODE_LINES : 0) | (k.pair ? SEGMODE_PAIR : 0);
}
// LDS of the k_seal_segments launch: the rest pass stages through EmitShiftLines only for SEGMODE_ANYIN
inline uint32_t seal_segments_lds(const Knobs &k)
{
    return seal_segments_two_pass(k) && !k.seal_ina ? 0u : WAVES * SHIFT_LDS_BYTES;
}
inline int open_segments_mode(const Knobs &k)
{
    return (k.seglines ? SEGMODE_LINES : 0) | (k.pair ? SEGMODE_PAIR : 0) | (k.shift16 ? SEGMODE_SHIFT16 : 0) |
           (k.open_ina ? SEGMODE_ANYIN : 0);
}
// czk_relay_segments: line-staged stores for the full waves of equal-length aligned segments
// (seglines), EmitShiftLines for those off the 128-byte lines (shift16); the rows' LDS only with lines
inline int relay_segments_mode(const Knobs &k)
{
    return (k.seglines ? SEGMODE_LINES : 0) | (k.shift16 ? SEGMODE_SHIFT16 : 0);
}
inline uint32_t relay_segments_lds(const Knobs &k) { return k.seglines ? WAVES * SHIFT_LDS_BYTES : 0u; }

}  // namespace czd
