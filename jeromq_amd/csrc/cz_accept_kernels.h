// cz_accept_kernels.h -- device side of the batched CURVE server handshake (cz_acceptor, section 11 of
// the header): HELLO -> WELCOME and INITIATE -> READY for many connections per launch.  Compiled as
// part of cz_x25519.hip, the handshake's device translation unit, on the box helpers and the
// per-lane-job X25519 kernel of cz_hs_dev.h.
//
// Reference: CurveServerMechanism.processHello :254-299, produceWelcome :301-358, processInitiate
// :360-471, produceReady :473-507.  Per connection the reference runs, through Curve.box / open /
// beforenm (Curve.java:124-193), the NaCl boxes that the kernels here run with one lane per
// connection, on keys that k_x25519_jobs lanes made:
//   k_acc_welcome   stage 1: open the HELLO box, seal the cookie and the WELCOME box, write the
//                   168-byte command and the slot's state record;
//   k_acc_initiate  stage 2a: open and check the cookie, open the INITIATE box;
//   k_acc_ready     stage 2b: open and check the vouch, seal the READY box.
// NaCl's rules and the access pattern: cz_hs_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_accept.h"
#include "cz_hs_dev.h"

namespace {

// Stage 1, one lane per well-formed HELLO.  in: CZA_IN1 records; x: the stage's three key
// agreements per record (S' = s'.9, k1 = beforenm(C', s), cnPrecom = beforenm(C', s')); out: CZA_OUT1
// records (status CZA_ST_NOT_RUN until a lane writes its own); state: the slot table.
__global__ __launch_bounds__(64) void k_acc_welcome(const uint8_t *__restrict__ in, const uint8_t *__restrict__ x,
                                                     uint8_t *__restrict__ out, uint8_t *__restrict__ state,
                                                     uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    const u32 *rec = words(in + (uint64_t)CZA_IN1 * j);
    const u32 *xr = words(x + (uint64_t)CZA_X1 * j);
    u32 *o = words(out + (uint64_t)CZA_OUT1 * j);
    u32 k1[8];
    ldw(k1, xr + 8);
    {   // Box [64 * %x0](C'->S) under nonce "CurveZMQHELLO---" + the client's 8 bytes: only the tag matters
        u32 d[16], tin[4], tag[4];
        ldw(tin, rec + CZA_IN1_BOX / 4);
        ldw(d, rec + CZA_IN1_BOX / 4 + 4);
        const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('H', 'E', 'L', 'L'), w4('O', '-', '-', '-'),
                          rec[CZA_IN1_NONCE / 4], rec[CZA_IN1_NONCE / 4 + 1]};
        xs_fixed<4, true>(d, tag, k1, n);
        if (diff<4>(tag, tin)) {
            o[0] = CZA_ST_CRYPTO;
            return;
        }
    }
    u32 cp[8], es[8], e[16];
    ldw(cp, rec + CZA_IN1_CP / 4);
    ldw(es, rec + CZA_IN1_SECRET / 4);
    ldw(e, rec + CZA_IN1_ENTROPY / 4);  // cookie nonce 16, cookie key 32, WELCOME nonce 16
    // cookie = secretbox [C' + s'] under the cookie key, nonce "COOKIE--" + 16 random bytes
    u32 m[16], ctag[4];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        m[i] = cp[i];
        m[8 + i] = es[i];
    }
    {
        const u32 n[6] = {w4('C', 'O', 'O', 'K'), w4('I', 'E', '-', '-'), e[0], e[1], e[2], e[3]};
        xs_fixed<4, false>(m, ctag, e + 4, n);
    }
    // WELCOME box [S' + cookie nonce + cookie](S->C') under k1, nonce "WELCOME-" + 16 random bytes
    u32 w[32], wtag[4];
#pragma unroll
    for (int i = 0; i < 8; i++)
        w[i] = xr[i];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[8 + i] = e[i];
        w[12 + i] = ctag[i];
    }
#pragma unroll
    for (int i = 0; i < 16; i++)
        w[16 + i] = m[i];
    {
        const u32 n[6] = {w4('W', 'E', 'L', 'C'), w4('O', 'M', 'E', '-'), e[12], e[13], e[14], e[15]};
        xs_fixed<8, false>(w, wtag, k1, n);
    }
    u32 *cmd = o + CZA_OUT1_CMD / 4;
    cmd[0] = w4('\x07', 'W', 'E', 'L');
    cmd[1] = w4('C', 'O', 'M', 'E');
#pragma unroll
    for (int i = 0; i < 4; i++) {
        cmd[2 + i] = e[12 + i];
        cmd[6 + i] = wtag[i];
    }
#pragma unroll
    for (int i = 0; i < 32; i++)
        cmd[10 + i] = w[i];
    // the slot's record: s', cookie key, cnPrecom, C'
    u32 *st = words(state + (uint64_t)CZA_STATE * rec[CZA_IN1_SLOT / 4]);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[CZA_STATE_SECRET / 4 + i] = es[i];
        st[CZA_STATE_COOKIE_KEY / 4 + i] = e[4 + i];
        st[CZA_STATE_PRECOM / 4 + i] = xr[16 + i];
        st[CZA_STATE_CP / 4 + i] = cp[i];
    }
    o[0] = CZA_ST_OK;
}

// Stage 2a, one lane per INITIATE that passed the host's size checks.  in: CZA_IN2 records; out:
// CZA_OUT2 records (status CZA_ST_NOT_RUN until a lane writes its own).  Opens the cookie under the slot's cookie key and
// compares its C' + s' with the slot's (the plaintext stays in registers), then opens the INITIATE
// box under cnPrecom into the record's plaintext area: C, the vouch nonce and box, the metadata.
__global__ __launch_bounds__(64) void k_acc_initiate(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                      const uint8_t *__restrict__ state, uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    const u32 *rec = words(in + (uint64_t)CZA_IN2 * j);
    u32 *o = words(out + (uint64_t)CZA_OUT2 * j);
    const u32 *st = words(state + (uint64_t)CZA_STATE * rec[CZA_IN2_SLOT / 4]);
    {
        u32 d[16], tin[4], tag[4], ck[8];
        ldw(tin, rec + CZA_IN2_COOKIE / 4);
        ldw(d, rec + CZA_IN2_COOKIE / 4 + 4);
        ldw(ck, st + CZA_STATE_COOKIE_KEY / 4);
        const u32 *cn = rec + CZA_IN2_COOKIE_NONCE / 4;
        const u32 n[6] = {w4('C', 'O', 'O', 'K'), w4('I', 'E', '-', '-'), cn[0], cn[1], cn[2], cn[3]};
        xs_fixed<4, true>(d, tag, ck, n);
        const u32 bad = diff<4>(tag, tin) | diff<8>(d, st + CZA_STATE_CP / 4) | diff<8>(d + 8, st + CZA_STATE_SECRET / 4);
        if (bad) {
            o[0] = CZA_ST_CRYPTO;
            return;
        }
    }
    u32 pre[8], tin[4], tag[4];
    ldw(pre, st + CZA_STATE_PRECOM / 4);
    ldw(tin, rec + CZA_IN2_BOX / 4);
    const u32 nbytes = rec[CZA_IN2_LEN / 4];  // 128 .. CZA_INIT_MAX, checked by the host side
    const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('I', 'N', 'I', 'T'), w4('I', 'A', 'T', 'E'),
                      rec[CZA_IN2_NONCE / 4], rec[CZA_IN2_NONCE / 4 + 1]};
    u32 *plain = o + CZA_OUT2_PLAIN / 4;
    xs_mem<true>(rec + CZA_IN2_BOX / 4 + 4, plain, nbytes, tag, pre, n);
    if (diff<4>(tag, tin)) {
        wipe_words(plain, (nbytes + 15u) / 16u * 4u);
        o[0] = CZA_ST_CRYPTO;
        return;
    }
    o[0] = CZA_ST_OK;
}

// Stage 2b, the same lanes after k_x25519_jobs gave k3 = beforenm(C, s') (32 bytes per lane in x).
// Opens the vouch Box [C',S](C->S') and compares its C' with the slot's, then seals the READY box
// [metadata](S'->C') under cnPrecom with nonce "CurveZMQREADY---" + BE64(1) and hands cnPrecom out.
// meta: the acceptor's metadata padded to whole 16-byte chunks.
__global__ __launch_bounds__(64) void k_acc_ready(uint8_t *__restrict__ out, const uint8_t *__restrict__ x,
                                                   const uint8_t *__restrict__ in, const uint8_t *__restrict__ state,
                                                   const uint8_t *__restrict__ meta, uint32_t meta_len, uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    u32 *o = words(out + (uint64_t)CZA_OUT2 * j);
    if (o[0] != CZA_ST_OK)
        return;
    const u32 *rec = words(in + (uint64_t)CZA_IN2 * j);
    const u32 *st = words(state + (uint64_t)CZA_STATE * rec[CZA_IN2_SLOT / 4]);
    u32 *plain = o + CZA_OUT2_PLAIN / 4;
    const u32 nwords = (rec[CZA_IN2_LEN / 4] + 15u) / 16u * 4u;
    {
        u32 d[16], tin[4], tag[4], k3[8];
        ldw(k3, words(x + 32ull * j));
        ldw(tin, plain + 12);  // C 32, vouch nonce 16, then the vouch box: tag 16, body 64
        ldw(d, plain + 16);
        const u32 n[6] = {w4('V', 'O', 'U', 'C'), w4('H', '-', '-', '-'), plain[8], plain[9], plain[10], plain[11]};
        xs_fixed<4, true>(d, tag, k3, n);
        if (diff<4>(tag, tin)) {
            wipe_words(plain, nwords);
            o[0] = CZA_ST_CRYPTO;
            return;
        }
        if (diff<8>(d, st + CZA_STATE_CP / 4)) {
            wipe_words(plain, nwords);
            o[0] = CZA_ST_KEY_EXCHANGE;
            return;
        }
    }
    u32 pre[8], tag[4];
    ldw(pre, st + CZA_STATE_PRECOM / 4);
    u32 *box = o + CZA_OUT2_READY / 4;
    if (meta_len) {
        const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('R', 'E', 'A', 'D'), w4('Y', '-', '-', '-'),
                          0u, 0x01000000u};
        xs_mem<false>(words(meta), box + 4, meta_len, tag, pre, n);
#pragma unroll
        for (int i = 0; i < 4; i++)
            box[i] = tag[i];
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        o[CZA_OUT2_PRECOM / 4 + i] = pre[i];
}

}  // namespace

extern "C" {

hipError_t czk_acc_welcome(const void *in, const void *x, void *out, void *state, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_acc_welcome, count, s, in, x, out, state, count);
}

hipError_t czk_acc_initiate(const void *in, void *out, const void *state, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_acc_initiate, count, s, in, out, state, count);
}

hipError_t czk_acc_ready(void *out, const void *x, const void *in, const void *state, const void *meta,
                         uint32_t meta_len, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_acc_ready, count, s, out, x, in, state, meta, meta_len, count);
}

}  // extern "C"
