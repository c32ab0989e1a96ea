// cz_relay_kernels.h -- CURVE relay: a received MESSAGE body re-sealed for another peer in one pass.
// Included by cz_kernels.hip inside its anonymous namespace (part 3), behind the emitters, open_frame
// and seal_frame whose parts it reuses; not a translation unit of its own.
//
// Reference path: Proxy.forward (zmq/Proxy.java:140-160), from.recv then to.send, is
// Mechanism.decode on one StreamEngine (CurveServerMechanism.java:165-225 /
// CurveClientMechanism.java:165-224) and Mechanism.encode on another (:126-163).
//
// The re-sealed body has the size and layout of the received one ("\x07MESSAGE" | nonce8 | tag16 | c),
// and body byte i is box byte i of both boxes, so from box byte 32 on c_out = c_in ^ ks_in ^ ks_out:
// no 33-byte funnel, no carried words, one load stream and one store stream, and the plaintext lives
// in registers only.  Per 64-byte block: load C, ks_in and Poly_in over C, ks_out, C' = C ^ ks_in ^
// ks_out (the flags byte masked to MORE | COMMAND in block 0, as a Msg keeps only those two bits:
// CurveServerMechanism.java:207-213 and :132-138), Poly_out over C', emit C'.
#pragma once

// waves per SIMD of the line-staged relay kernel (two keystream blocks and two Poly1305 chains per lane)
#ifndef CZ_RELAY_WAVES_PER_EU
#define CZ_RELAY_WAVES_PER_EU 3
#endif
#define CZ_RELAY_OCC __attribute__((amdgpu_waves_per_eu(CZ_RELAY_WAVES_PER_EU, CZ_RELAY_WAVES_PER_EU)))

// RELAY one frame: in = MESSAGE body (size bytes) under kin, the emitter receives the MESSAGE body of
// the same size under kout with nonce counter_out.  Returns open_frame's CZ_STATUS_* for the inbound
// body (*flags_out = the decrypted flags byte, *nonce_out = the inbound wire nonce, set as open_frame
// sets them); for every status but OK the emitter's `size` bytes end as zeros (em.close(true)): a frame
// rejected before decryption emits nothing else, a bad tag is found after the body was emitted.
// `in` and the emitter's output may be the same bytes (EmitDirect): every block, the header and the
// tag are loaded before anything is stored over them, and neither pointer is __restrict__.
// INA: the input's alignment class, as open_frame (16: AL as given; 8 / 1 with AL: dword-aligned loads).
// The kernels below instantiate 16 only: 8 / 1 are the loads of a line-staged dense relay, which is open
// (DESIGN.md section 8).
//
// SEG (relay_segment): the same block loop over box blocks [sg->b0, min(sg->b1, nblk)) of a body whose
// header passed open_header (nonce words sg->n0, sg->n1; check_floor, floor and nonce_out are not
// used).  Output chunk q is box block b0 + q at the emitter's base (out body + 64 * b0), the seal
// segment's geometry.  Both Poly1305 states are keyed from keystream block 0 of their own side,
// recomputed per segment as open_segment and seal_segment do.  sg->rec_in == nullptr: the whole frame,
// finished as above (CZ_STATUS_OK or CZ_STATUS_CRYPTO).  Otherwise the inbound partial goes to rec_in
// (open_segment's record: h, the Poly block count, and from the block-0 segment the flags byte in [6]
// and r, pad in [8..15]; [7] is the kernel's), the outbound one to rec_out (seal_segment's record), the
// tag slot is left to the combine, and the return is CZ_STATUS_OK.  The emit site is one for every
// lane: a cooperative emitter's wave may hold block-0 segments and later ones side by side.
struct RelaySeg {
    u32 n0, n1, b0, b1;
    u32 *rec_in, *rec_out;
};
template <bool AL, class EM, int INA = 16, bool SEG = false>
__device__ __forceinline__ u32 relay_frame(const uint8_t *in, u32 size, const u32 kin[8], bool check_floor,
                                           long long floor, const u32 kout[8], u64 counter_out, u32 *flags_out,
                                           u64 *nonce_out, EM &em, const RelaySeg *sg = nullptr)
{
    static_assert(INA == 16 || (AL && (INA == 8 || INA == 1)), "INA 8/1 take the AL code paths");
    const u32 ina = INA == 1 ? (u32)(uintptr_t)in & 3u : 0u;
    const uint8_t *in4 = in - ina;
    // the 16 box bytes at `off`, every one inside the body
    auto LF = [&](u32 off) -> V4 {
        if constexpr (INA == 16) {
            return ld16f<AL>(in + off);
        } else {
            const uint4 r = *reinterpret_cast<const u4_a4 *>(in4 + off);
            if constexpr (INA == 8)
                return V4{r.x, r.y, r.z, r.w};
            const u32 r4 = ina ? *reinterpret_cast<const u32 *>(in4 + off + 16) : 0u;
            return V4{funnel(r.y, r.x, ina), funnel(r.z, r.y, ina), funnel(r.w, r.z, ina), funnel(r4, r.w, ina)};
        }
    };
    // the box bytes at `off`, avail of them inside the body
    auto LP = [&](u32 off, u64 avail) -> V4 {
        if constexpr (INA == 16)
            return ld16<AL>(in + off, avail);
        else
            return avail >= 16u ? LF(off) : ld16<false>(in + off, avail);
    };
    constexpr bool COOP = EM::cooperative;
    // header, size and floor: open_frame's checks (Msgs.startsWith never reaches byte 7)
    u32 early = CZ_STATUS_OK;
    const V4 h = SEG ? V4{HDR0, HDR1, sg->n0, sg->n1} : LP(0, size);
    if (size < 8u || h.x != HDR0 || (h.y & 0x00ffffffu) != (HDR1 & 0x00ffffffu))
        early = CZ_STATUS_COMMAND;
    else if (size < 33u)
        early = CZ_STATUS_MALFORMED;
    const u32 n0 = h.z, n1 = h.w;
    if (!SEG && early == CZ_STATUS_OK) {
        const u64 nonce = ((u64)bswap32(n0) << 32) | (u64)bswap32(n1);
        *nonce_out = nonce;
        if (check_floor && (long long)nonce <= floor)
            early = CZ_STATUS_SEQUENCE;
    }
    if (early != CZ_STATUS_OK && !COOP) {
        em.close(true);  // rejected before decryption: zeros over the body's bytes
        return early;
    }
    if (size < 33u)
        return early;  // (cooperative callers only launch sizes >= LINES_BYTES_MIN)
    // a cooperative emitter needs every lane in the same chunk sequence: a rejected frame runs the
    // loop as a dead lane, and close() zeroes what it emitted
    const bool dead = early != CZ_STATUS_OK;
    u32 m0, m1;
    counter_nonce(counter_out, m0, m1);

    const u32 nblk = (size + 63u) >> 6;
    const u32 nfull = size >> 6;
    // SEG: box blocks [b0, bend); first: this lane holds block 0
    const u32 b0 = SEG ? sg->b0 : 0u;
    const u32 bend = SEG && sg->b1 < nblk ? sg->b1 : nblk;
    const bool first = !SEG || b0 == 0u;
    u32 mpoly = 0;  // SEG: 16-byte Poly1305 blocks absorbed, the same on both sides (open_segment's count)
    u32 x[16], C[16];
    Poly Pi, Po;

    // block 0: keystream bytes 0..31 key the MACs, box bytes 32..63 are the flags byte and payload
    salsa20_block<true>(x, kin, n0, n1, 0u, 0u);
    poly_init(Pi, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
    const V4 tin = first ? LP(16, size - 16u) : zero4();
    if (first) {
        const V4 a = LP(32, size - 32u);
        const V4 b = LP(48, size > 48u ? size - 48u : 0u);
        C[8] = a.x; C[9] = a.y; C[10] = a.z; C[11] = a.w;
        C[12] = b.x; C[13] = b.y; C[14] = b.z; C[15] = b.w;
    }
    // Poly1305 over box bytes 32.. of block 0 (nb = min(size, 64) - 32 of them)
    auto poly_block0 = [&](Poly &P) {
        if (nfull >= 1) {
            poly_block(P, C[8], C[9], C[10], C[11], 1u);
            poly_block(P, C[12], C[13], C[14], C[15], 1u);
        } else {
            const u32 nb = size - 32u;
            if (nb >= 16u) {
                poly_block(P, C[8], C[9], C[10], C[11], 1u);
                if (nb > 16u)
                    poly_block_partial(P, C[12], C[13], C[14], C[15], nb - 16u);
            } else {
                poly_block_partial(P, C[8], C[9], C[10], C[11], nb);
            }
        }
    };
    if (first) {
        poly_block0(Pi);
#pragma unroll
        for (int k = 8; k < 16; k++)
            C[k] ^= x[k];  // plaintext, in registers only
        *flags_out = C[8] & 0xffu;
        C[8] &= 0xffffff00u | (CZ_MSG_MORE | CZ_MSG_COMMAND);
        if constexpr (SEG)
            mpoly = ((size < 64u ? size : 64u) - 32u + 15u) >> 4;
    }
    salsa20_block<true>(x, kout, m0, m1, 0u, 0u);
    poly_init(Po, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
    if (first) {
#pragma unroll
        for (int k = 8; k < 16; k++)
            C[k] ^= x[k];
        poly_block0(Po);
        C[0] = HDR0; C[1] = HDR1; C[2] = m0; C[3] = m1;
        C[4] = C[5] = C[6] = C[7] = 0u;  // tag slot, written by em.tag() (SEG: or by the combine)
    }
    if constexpr (!SEG)
        em.emit(0, C);

    // Poly1305 over block blk's ciphertext in C (tailv of its 64 bytes are body)
    auto poly_blockn = [&](Poly &P, bool full, u32 tailv) {
        if (full) {
            poly_block(P, C[0], C[1], C[2], C[3], 1u);
            poly_block(P, C[4], C[5], C[6], C[7], 1u);
            poly_block(P, C[8], C[9], C[10], C[11], 1u);
            poly_block(P, C[12], C[13], C[14], C[15], 1u);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32 s = 16u * j;
                if (s < tailv) {
                    const u32 nb = tailv - s;
                    if (nb >= 16)
                        poly_block(P, C[4 * j], C[4 * j + 1], C[4 * j + 2], C[4 * j + 3], 1u);
                    else
                        poly_block_partial(P, C[4 * j], C[4 * j + 1], C[4 * j + 2], C[4 * j + 3], nb);
                }
            }
        }
    };
    for (u32 blk = SEG ? b0 : 1u; blk < bend; blk++) {
        const bool full = blk < nfull;
        const u32 o = 64u * blk, tailv = size - o;
        if (!SEG || blk != 0u) {
            V4 q0, q1, q2, q3;
            if (full) {
                q0 = LF(o);
                q1 = LF(o + 16u);
                q2 = LF(o + 32u);
                q3 = LF(o + 48u);
            } else {
                q0 = LP(o, tailv);
                q1 = LP(o + 16u, tailv > 16u ? tailv - 16u : 0u);
                q2 = LP(o + 32u, tailv > 32u ? tailv - 32u : 0u);
                q3 = LP(o + 48u, tailv > 48u ? tailv - 48u : 0u);
            }
            C[0] = q0.x; C[1] = q0.y; C[2] = q0.z; C[3] = q0.w;
            C[4] = q1.x; C[5] = q1.y; C[6] = q1.z; C[7] = q1.w;
            C[8] = q2.x; C[9] = q2.y; C[10] = q2.z; C[11] = q2.w;
            C[12] = q3.x; C[13] = q3.y; C[14] = q3.z; C[15] = q3.w;
            // a last block of at most 16 body bytes: keystream words 0..3 only, on both sides (the bytes
            // of words 4..15 are past the body: masked by Poly1305's partial block and by the emitter)
            const bool w03 = !full && tailv <= 16u;
            if (w03)
                salsa20_block_w03<true>(x, kin, n0, n1, blk, 0u);
            else
                salsa20_block<true>(x, kin, n0, n1, blk, 0u);
            poly_blockn(Pi, full, tailv);
#pragma unroll
            for (int k = 0; k < 16; k++)
                C[k] ^= x[k];
            if (w03)
                salsa20_block_w03<true>(x, kout, m0, m1, blk, 0u);
            else
                salsa20_block<true>(x, kout, m0, m1, blk, 0u);
#pragma unroll
            for (int k = 0; k < 16; k++)
                C[k] ^= x[k];
            poly_blockn(Po, full, tailv);
            if constexpr (SEG)
                mpoly += full ? 4u : (tailv + 15u) >> 4;
        }
        if constexpr (SEG)
            em.emit(blk - b0, C);  // (block 0 of a first segment: C as left above)
        else if (full)
            em.emit_full(blk, C);
        else
            em.emit(blk, C);
    }

    // (one tag() / close() site: a cooperative wave may hold whole frames and segments side by side)
    u32 diff = 0;
    if (!SEG || !sg->rec_in) {
        u32 tag[4];
        poly_finish(Pi, tag);
        diff = (tag[0] ^ tin.x) | (tag[1] ^ tin.y) | (tag[2] ^ tin.z) | (tag[3] ^ tin.w);
        poly_finish(Po, tag);
        em.tag(tag);
    }
    // never leave a sealed copy of unauthenticated plaintext; converged for cooperative emitters
    em.close(dead || diff != 0);
    if constexpr (SEG) {
        if (sg->rec_in) {
            u32 *ri = sg->rec_in, *ro = sg->rec_out;
            ri[0] = Pi.h0; ri[1] = Pi.h1; ri[2] = Pi.h2; ri[3] = Pi.h3; ri[4] = Pi.h4; ri[5] = mpoly;
            ro[0] = Po.h0; ro[1] = Po.h1; ro[2] = Po.h2; ro[3] = Po.h3; ro[4] = Po.h4; ro[5] = mpoly;
            if (first) {
                ri[6] = *flags_out;
                ri[8] = Pi.r0; ri[9] = Pi.r1; ri[10] = Pi.r2; ri[11] = Pi.r3;
                ri[12] = Pi.p0; ri[13] = Pi.p1; ri[14] = Pi.p2; ri[15] = Pi.p3;
                ro[8] = Po.r0; ro[9] = Po.r1; ro[10] = Po.r2; ro[11] = Po.r3;
                ro[12] = Po.p0; ro[13] = Po.p1; ro[14] = Po.p2; ro[15] = Po.p3;
            }
            return CZ_STATUS_OK;
        }
    }
    if (dead)
        return early;
    return diff != 0 ? (u32)CZ_STATUS_CRYPTO : (u32)CZ_STATUS_OK;
}

// RELAY box blocks [b0, b1) of one body whose header passed open_header: relay_frame's SEG form
template <bool AL, class EM>
__device__ __forceinline__ u32 relay_segment(const uint8_t *in, u32 size, const u32 kin[8], u32 n0, u32 n1,
                                             const u32 kout[8], u64 counter_out, u32 b0, u32 b1, u32 *rec_in,
                                             u32 *rec_out, u32 &flags_out, EM &em)
{
    const RelaySeg sg{n0, n1, b0, b1, rec_in, rec_out};
    u64 nonce = 0;
    return relay_frame<AL, EM, 16, true>(in, size, kin, false, 0, kout, counter_out, &flags_out, &nonce, em, &sg);
}

// One lane of a relay whose output is stored lane by lane: AL code paths when body and output both
// sit on 16 bytes, unaligned 16-byte loads and byte-exact stores otherwise
__device__ __forceinline__ u32 relay_direct(const uint8_t *src, uint8_t *dst, u32 size, const u32 kin[8], bool check,
                                            long long floor, const u32 kout[8], u64 counter, u32 *fl, u64 *nonce)
{
    if (aligned16(src, dst)) {
        EmitDirect<true> em{dst, size};
        return relay_frame<true, EmitDirect<true>>(src, size, kin, check, floor, kout, counter, fl, nonce, em);
    }
    EmitDirect<false> em{dst, size};
    return relay_frame<false, EmitDirect<false>>(src, size, kin, check, floor, kout, counter, fl, nonce, em);
}

// cz_relay_batch: one lane per frame.  desc[i] as k_open_desc reads it (out_off: the re-sealed body),
// to[i] = the outbound {counter, key_idx}.  status / nonces as k_open_desc.
__global__ __launch_bounds__(BLOCK) void k_relay_desc(const cz_frame_desc *__restrict__ desc,
                                                       const cz_fanout_sub *__restrict__ to,
                                                       const uint32_t *__restrict__ order, uint32_t count,
                                                       const uint8_t *in, uint8_t *out,
                                                       const uint8_t *__restrict__ subkeys,
                                                       uint16_t *__restrict__ status, uint64_t *__restrict__ nonces)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= count)
        return;
    const uint32_t i = order ? order[t] : t;
    const cz_frame_desc d = desc[i];
    const cz_fanout_sub sb = to[i];
    u32 kin[8], kout[8];
    load_key(subkeys + 32ull * d.key_idx, kin);
    load_key(subkeys + 32ull * sb.key_idx, kout);
    long long floor = (long long)d.counter;
    if (d.prev >= 0) {
        // replay floor = nonce of the previous frame of this connection in the batch (out of place
        // only: in place, another lane may already have re-sealed that body)
        const cz_frame_desc p = desc[d.prev];
        floor = (long long)read_be64(in + p.in_off + 8);
    }
    u32 fl = 0;
    u64 nonce = 0;
    const u32 st = relay_direct(in + d.in_off, out + d.out_off, d.len, kin, (d.flags & CZ_DESC_CHECK_NONCE) != 0, floor,
                                kout, sb.counter, &fl, &nonce);
    status[i] = (uint16_t)(st | (st == CZ_STATUS_OK ? (fl << 8) : 0u));
    if (nonces)
        nonces[i] = nonce;
}

// cz_relay_uniform: one connection's bodies in order (frame i must beat frame i - 1's wire nonce,
// frame 0 floor0; prev0: frame 0's floor is the body in_stride bytes before it -- the lane-wise tail
// behind a line-staged head) re-sealed for one connection with nonce counter0 + i.
// ST_LINES: full waves only, everything on 16 bytes, out_stride a line multiple: the seal's line
// emitter.  ST_DIRECT: lane-wise and byte-exact at every layout.  Both write the zeros an owning
// out_stride (czd::owns_slots) is owed past each body themselves: no zero-pad launch.
template <int ST>
__global__ __launch_bounds__(BLOCK) CZ_RELAY_OCC void k_relay_uniform(
    const uint8_t *in, uint64_t in_stride, uint8_t *out, uint64_t out_stride, uint32_t count, uint32_t size,
    const uint8_t *__restrict__ subkey_in, uint64_t floor0, int check, const uint8_t *__restrict__ subkey_out,
    uint64_t counter0, uint16_t *__restrict__ status, int prev0)
{
    static_assert(ST == ST_LINES || ST == ST_DIRECT, "relay: the line emitter or lane-wise stores");
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if constexpr (ST == ST_LINES) {
        if ((i & ~63u) + 64u > count)
            return;  // (the launcher sends the frames behind the last full wave to ST_DIRECT)
    } else {
        if (i >= count)
            return;
    }
    // both keys are wave-uniform: scalar loads, SGPRs
    u32 kin[8], kout[8];
    load_key(subkey_in, kin);
    load_key(subkey_out, kout);
    const uint8_t *src = in + (uint64_t)i * in_stride;
    uint8_t *dst = out + (uint64_t)i * out_stride;
    u32 fl = 0;
    u64 nonce = 0;
    u32 st;
    if constexpr (ST == ST_LINES) {
        extern __shared__ uint4 smem[];
        long long floor = (long long)floor0;
        if (i > 0 || prev0) {
            const uint2 pn = *reinterpret_cast<const uint2 *>(src - in_stride + 8);
            floor = (long long)(((u64)bswap32(pn.x) << 32) | (u64)bswap32(pn.y));
        }
        using EmL = EmitLinesSeal;
        EmL em{smem + (threadIdx.x >> 6) * (LINE_LDS_BYTES / 16), out + (uint64_t)(i & ~63u) * out_stride, dst,
               out_stride, threadIdx.x & 63u, size, 0u, true,
               smem + (WAVES * LINE_LDS_BYTES + (threadIdx.x >> 6) * HOLD_LDS_BYTES) / 16};
        st = relay_frame<true, EmL>(src, size, kin, check != 0, floor, kout, counter0 + i, &fl, &nonce, em);
        // EmitLines ends at the body's last line; a slot with more lines than that is owned too
        const u32 body_lines = (size + 127u) & ~127u;
        if (out_stride > body_lines)
            zero_bytes(dst + body_lines, (u32)(out_stride - body_lines));
    } else {
        const long long floor = (i > 0 || prev0) ? (long long)read_be64(src - in_stride + 8) : (long long)floor0;
        st = relay_direct(src, dst, size, kin, check != 0, floor, kout, counter0 + i, &fl, &nonce);
        if (fanout_owns(out_stride) && out_stride > size)
            zero_bytes(dst + size, (u32)(out_stride - size));
    }
    status[i] = (uint16_t)(st | (st == CZ_STATUS_OK ? (fl << 8) : 0u));
}

// ---- segmented relay (header section 3i): long bodies re-sealed across lanes ----------------------
// waves per SIMD of k_relay_segments: two keys, two keystream blocks and two Poly1305 chains per lane, as
// k_relay_desc (189 VGPRs); DESIGN.md section 4 "Segmented relay" records what this compiles to
#ifndef CZ_RELAY_SEG_WAVES_PER_EU
#define CZ_RELAY_SEG_WAVES_PER_EU 2
#endif
#define CZ_RELAY_SEG_OCC __attribute__((amdgpu_waves_per_eu(CZ_RELAY_SEG_WAVES_PER_EU, CZ_RELAY_SEG_WAVES_PER_EU)))

// cz_relay_segments: one lane per segment, structured as k_open_segments.  Every lane runs open_header
// for its frame (floor from desc[prev]'s body in `in`); the lane with block 0 writes the nonce, rec[7] =
// early for the combine, and an early status.  work: two planes of npart records, the inbound partial
// of part p at record p (open_segment's layout), the outbound one at record npart + p.
// A full wave of segments with one chunk count, bodies and outputs on 16 bytes and no rejected lane
// takes a seal line emitter (EmitSegLines, or with SEGMODE_SHIFT16 and outputs off the 128-byte lines
// EmitShiftLines); every other wave stores lane by lane, byte-exact at any alignment of either side.
// A frame rejected before decryption: each of its segments zeroes its own byte range.
__global__ __launch_bounds__(BLOCK) CZ_RELAY_SEG_OCC void k_relay_segments(
    const cz_frame_desc *__restrict__ desc, const cz_fanout_sub *__restrict__ to, const cz_segment *__restrict__ segs,
    uint32_t nseg, const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint8_t *__restrict__ subkeys,
    u32 *__restrict__ work, uint32_t npart, uint16_t *__restrict__ status, uint64_t *__restrict__ nonces, int mode)
{
    extern __shared__ uint4 smem[];
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t wave_first = t & ~63u;
    if (wave_first >= nseg)
        return;
    const bool live = t < nseg;
    const cz_segment sg = segs[live ? t : wave_first];
    const cz_frame_desc d = desc[sg.frame];
    const cz_fanout_sub sb = to[sg.frame];
    long long floor = (long long)d.counter;
    if (d.prev >= 0)
        floor = (long long)read_be64(in + desc[d.prev].in_off + 8);
    const uint8_t *src = in + d.in_off;
    u32 n0 = 0, n1 = 0;
    u64 nonce = 0;
    const u32 early = open_header(src, d.len, (d.flags & CZ_DESC_CHECK_NONCE) != 0, floor, n0, n1, nonce);
    u32 *rec_in = sg.part == 0xffffffffu ? nullptr : work + 16ull * sg.part;
    u32 *rec_out = rec_in ? rec_in + 16ull * npart : nullptr;
    if (live && sg.first_block == 0) {
        if (nonces)
            nonces[sg.frame] = nonce;
        if (rec_in)
            rec_in[7] = early;  // the combine kernel finishes frames whose header passed
        if (early != CZ_STATUS_OK)
            status[sg.frame] = (uint16_t)early;
    }
    // this segment's bytes: box blocks [first_block, bend) of the body, clipped to its size
    const u32 nblk = (d.len + 63u) >> 6;
    const u32 b1 = sg.first_block + sg.nblocks;
    const u32 bend = b1 < nblk ? b1 : nblk;
    const u64 end = 64ull * bend < d.len ? 64ull * bend : d.len;
    const u32 total = end > 64ull * sg.first_block ? (u32)(end - 64ull * sg.first_block) : 0u;
    const u32 nch = (total + 63u) >> 6;
    uint8_t *dst = out + d.out_off + 64ull * sg.first_block;
    const bool al = aligned16(src, dst);
    u32 key_in[8], key_out[8];
    load_key(subkeys + 32ull * d.key_idx, key_in);
    load_key(subkeys + 32ull * sb.key_idx, key_out);
    u32 fl = 0, st;
    if ((mode & SEGMODE_LINES) && wave_lines_ok(wave_first + 64u <= nseg, nch, al) &&
        __builtin_amdgcn_ballot_w64(early != CZ_STATUS_OK || nch == 0u) == 0) {
        const u32 lane = threadIdx.x & 63u;
        uint8_t *wl = reinterpret_cast<uint8_t *>(smem) + (threadIdx.x >> 6) * SHIFT_LDS_BYTES;
        const bool line_al = (((uintptr_t)dst) & 127u) == 0;  // as in seal_segments_body
        if (!(mode & SEGMODE_SHIFT16) || __builtin_amdgcn_ballot_w64(!line_al) == 0) {
            EmitSegLinesSeal em{reinterpret_cast<uint4 *>(wl), dst, lane, total, 0u, 0u};
            em.init(sg.first_block == 0);
            st = relay_segment<true>(src, d.len, key_in, n0, n1, key_out, sb.counter, sg.first_block, b1, rec_in,
                                     rec_out, fl, em);
        } else {
            EmitShiftLinesSeal em{wl, dst, lane, total, 0u, 0u};
            em.init(sg.first_block == 0);
            st = relay_segment<true>(src, d.len, key_in, n0, n1, key_out, sb.counter, sg.first_block, b1, rec_in,
                                     rec_out, fl, em);
        }
    } else {
        if (!live)
            return;
        if (early != CZ_STATUS_OK || nch == 0u) {
            zero_bytes(dst, total);  // rejected before decryption: zeros over this segment's bytes
            return;
        }
        if (al) {
            EmitDirect<true> em{dst, total};
            st = relay_segment<true>(src, d.len, key_in, n0, n1, key_out, sb.counter, sg.first_block, b1, rec_in,
                                     rec_out, fl, em);
        } else {
            EmitDirect<false> em{dst, total};
            st = relay_segment<false>(src, d.len, key_in, n0, n1, key_out, sb.counter, sg.first_block, b1, rec_in,
                                      rec_out, fl, em);
        }
    }
    if (!rec_in)
        status[sg.frame] = (uint16_t)(st | (st == CZ_STATUS_OK ? (fl << 8) : 0u));
}

// One lane per split frame: combine_tag over the inbound plane against the received tag; a match
// joins the outbound plane into the tag slot the segments left, a mismatch zeroes the whole body
// (16-byte stores over the aligned interior, as k_open_combine) -- no sealed copy of unauthenticated
// plaintext outlives this kernel.  A frame rejected before decryption (rec[7]) is finished already.
__global__ __launch_bounds__(BLOCK) void k_relay_combine(const cz_frame_desc *__restrict__ desc,
                                                          const cz_combine *__restrict__ comb, uint32_t ncomb,
                                                          const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                          const u32 *__restrict__ work, uint32_t npart,
                                                          uint16_t *__restrict__ status)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= ncomb)
        return;
    const cz_combine cb = comb[t];
    const u32 *Ri = work + 16ull * cb.part0;
    if (Ri[7] != CZ_STATUS_OK)
        return;
    const cz_frame_desc d = desc[cb.frame];
    u32 tag[4];
    combine_tag(Ri, cb.nseg, tag);
    const uint8_t *tp = in + d.in_off + 16;
    u32 tin[4];
    for (int w = 0; w < 4; w++)
        tin[w] = (u32)tp[4 * w] | ((u32)tp[4 * w + 1] << 8) | ((u32)tp[4 * w + 2] << 16) |
                 ((u32)tp[4 * w + 3] << 24);
    if ((tag[0] ^ tin[0]) | (tag[1] ^ tin[1]) | (tag[2] ^ tin[2]) | (tag[3] ^ tin[3])) {
        zero_bytes(out + d.out_off, d.len);
        status[cb.frame] = CZ_STATUS_CRYPTO;
        return;
    }
    combine_tag(Ri + 16ull * npart, cb.nseg, tag);
    uint8_t *dst = out + d.out_off + 16;
    if ((((uintptr_t)dst) & 15u) == 0)
        st16<true>(dst, tag[0], tag[1], tag[2], tag[3]);
    else
        st16<false>(dst, tag[0], tag[1], tag[2], tag[3]);
    status[cb.frame] = (uint16_t)(CZ_STATUS_OK | (Ri[6] << 8));
}
