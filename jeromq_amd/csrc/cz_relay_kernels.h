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
template <bool AL, class EM, int INA = 16>
__device__ __forceinline__ u32 relay_frame(const uint8_t *in, u32 size, const u32 kin[8], bool check_floor,
                                           long long floor, const u32 kout[8], u64 counter_out, u32 *flags_out,
                                           u64 *nonce_out, EM &em)
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
    const V4 h = LP(0, size);
    if (size < 8u || h.x != HDR0 || (h.y & 0x00ffffffu) != (HDR1 & 0x00ffffffu))
        early = CZ_STATUS_COMMAND;
    else if (size < 33u)
        early = CZ_STATUS_MALFORMED;
    const u32 n0 = h.z, n1 = h.w;
    if (early == CZ_STATUS_OK) {
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
    u32 x[16], C[16];
    Poly Pi, Po;

    // block 0: keystream bytes 0..31 key the MACs, box bytes 32..63 are the flags byte and payload
    salsa20_block<true>(x, kin, n0, n1, 0u, 0u);
    poly_init(Pi, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
    const V4 tin = LP(16, size - 16u);
    {
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
    poly_block0(Pi);
#pragma unroll
    for (int k = 8; k < 16; k++)
        C[k] ^= x[k];  // plaintext, in registers only
    *flags_out = C[8] & 0xffu;
    C[8] &= 0xffffff00u | (CZ_MSG_MORE | CZ_MSG_COMMAND);
    salsa20_block<true>(x, kout, m0, m1, 0u, 0u);
    poly_init(Po, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
#pragma unroll
    for (int k = 8; k < 16; k++)
        C[k] ^= x[k];
    poly_block0(Po);
    C[0] = HDR0; C[1] = HDR1; C[2] = m0; C[3] = m1;
    C[4] = C[5] = C[6] = C[7] = 0u;  // tag slot, written by em.tag()
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
    for (u32 blk = 1; blk < nblk; blk++) {
        const bool full = blk < nfull;
        const u32 o = 64u * blk, tailv = size - o;
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
        if (full)
            em.emit_full(blk, C);
        else
            em.emit(blk, C);
    }

    u32 tag[4];
    poly_finish(Pi, tag);
    const u32 diff = (tag[0] ^ tin.x) | (tag[1] ^ tin.y) | (tag[2] ^ tin.z) | (tag[3] ^ tin.w);
    poly_finish(Po, tag);
    em.tag(tag);
    // never leave a sealed copy of unauthenticated plaintext; converged for cooperative emitters
    em.close(dead || diff != 0);
    if (dead)
        return early;
    return diff != 0 ? (u32)CZ_STATUS_CRYPTO : (u32)CZ_STATUS_OK;
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
