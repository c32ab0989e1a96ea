// cz_connect_kernels.h -- device side of the batched CURVE client handshake (cz_connector, section 12
// of the header): HELLO, WELCOME -> INITIATE and READY for many connections per launch.  Compiled as
// part of cz_x25519.hip, the handshake's device translation unit, on the box helpers and the
// per-lane-job X25519 kernel of cz_hs_dev.h.
//
// Reference: CurveClientMechanism.produceHello :246-279, processWelcome :281-316, produceInitiate
// :318-385, processReady :387-419.  Per connection the reference runs, through Curve.box / open /
// beforenm (Curve.java:124-193), the NaCl boxes that the kernels here run with one lane per
// connection, on keys that k_x25519_jobs lanes made:
//   k_con_hello     stage 1: seal Box [64 * %x0](C'->S) under kH, write the 200-byte HELLO and the
//                   slot's state record (c', kH);
//   k_con_welcome   stage 2a: open the WELCOME box under kH, hand out S' and the cookie;
//   k_con_initiate  stage 2b: seal the vouch under kV and the INITIATE box under cnPrecom, write the
//                   command, wipe c', kH and kV from the slot;
//   k_con_ready     stage 3: open the READY box under cnPrecom.
// NaCl's rules and the access pattern: cz_hs_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_connect.h"
#include "cz_hs_dev.h"

namespace {

// Stage 1, one lane per connection that got a slot.  in: CZC_IN1 records; x: the stage's two key
// agreements per record (C' = c'.9, kH = beforenm(S, c')); out: CZC_OUT1 records; state: the slot table.
__global__ __launch_bounds__(64) void k_con_hello(const uint8_t *__restrict__ in, const uint8_t *__restrict__ x,
                                                   uint8_t *__restrict__ out, uint8_t *__restrict__ state,
                                                   uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    const u32 *rec = words(in + (uint64_t)CZC_IN1 * j);
    const u32 *xr = words(x + (uint64_t)CZC_X1 * j);
    u32 *o = words(out + (uint64_t)CZC_OUT1 * j);
    u32 kh[8], es[8];
    ldw(kh, xr + 8);
    ldw(es, rec + CZC_IN1_SECRET / 4);
    // Box [64 * %x0](C'->S) under nonce "CurveZMQHELLO---" + BE64(1)
    u32 d[16], tag[4];
#pragma unroll
    for (int i = 0; i < 16; i++)
        d[i] = 0u;
    {
        const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('H', 'E', 'L', 'L'), w4('O', '-', '-', '-'),
                          0u, 0x01000000u};
        xs_fixed<4, false>(d, tag, kh, n);
    }
    // "\x05HELLO" 1 0 | 72 zero bytes | C' | nonce | tag | box
    u32 *cmd = o + CZC_OUT1_CMD / 4;
    cmd[0] = w4('\x05', 'H', 'E', 'L');
    cmd[1] = w4('L', 'O', '\x01', '\x00');
#pragma unroll
    for (int i = 2; i < 20; i++)
        cmd[i] = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++)
        cmd[20 + i] = xr[i];
    cmd[28] = 0u;
    cmd[29] = 0x01000000u;
#pragma unroll
    for (int i = 0; i < 4; i++)
        cmd[30 + i] = tag[i];
#pragma unroll
    for (int i = 0; i < 16; i++)
        cmd[34 + i] = d[i];
    // the slot's record: c' and kH (cnPrecom and kV are stage 2's)
    u32 *st = words(state + (uint64_t)CZC_STATE * rec[CZC_IN1_SLOT / 4]);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[CZC_STATE_SECRET / 4 + i] = es[i];
        st[CZC_STATE_KH / 4 + i] = kh[i];
        st[CZC_STATE_PRECOM / 4 + i] = 0u;
        st[CZC_STATE_KV / 4 + i] = 0u;
    }
    o[0] = CZA_ST_OK;
}

// Stage 2a, one lane per WELCOME of the right size.  in: CZC_IN2 records; out: CZC_OUT2 records (status
// CZA_ST_NOT_RUN until a lane writes its own); x: CZC_X2 scratch records.  Opens Box [S' + cookie](S->C')
// under the slot's kH and nonce "WELCOME-" + the command's 16 bytes; S' goes to the scratch record (the
// point of the stage's two key agreements), the cookie straight into the INITIATE command.
__global__ __launch_bounds__(64) void k_con_welcome(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                     uint8_t *__restrict__ x, const uint8_t *__restrict__ state,
                                                     uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    const u32 *rec = words(in + (uint64_t)CZC_IN2 * j);
    u32 *o = words(out + (uint64_t)CZC_OUT2 * j);
    const u32 *st = words(state + (uint64_t)CZC_STATE * rec[CZC_IN2_SLOT / 4]);
    u32 kh[8], d[32], tin[4], tag[4];
    ldw(kh, st + CZC_STATE_KH / 4);
    ldw(tin, rec + CZC_IN2_BOX / 4);
    ldw(d, rec + CZC_IN2_BOX / 4 + 4);
    const u32 *wn = rec + CZC_IN2_NONCE / 4;
    const u32 n[6] = {w4('W', 'E', 'L', 'C'), w4('O', 'M', 'E', '-'), wn[0], wn[1], wn[2], wn[3]};
    xs_fixed<8, true>(d, tag, kh, n);
    if (diff<4>(tag, tin)) {
        o[0] = CZA_ST_CRYPTO;
        return;
    }
    u32 *sp = words(x + (uint64_t)CZC_X2 * j + CZC_X2_SP);
#pragma unroll
    for (int i = 0; i < 8; i++)
        sp[i] = d[i];
    u32 *cookie = o + (CZC_OUT2_CMD + 9) / 4;
#pragma unroll
    for (int i = 0; i < 24; i++)
        cookie[i] = d[8 + i];
    o[0] = CZA_ST_OK;
}

// Stage 2b, the same lanes after k_x25519_jobs wrote cnPrecom = beforenm(S', c') and kV = beforenm(S', c)
// into the slot.  Seals the vouch Box [C' + S](c->S') under "VOUCH---" + 16 random bytes, then
// Box [C + vouch nonce + vouch + metadata](C'->S') under "CurveZMQINITIATE" + BE64(2), and completes the
// command k_con_welcome put the cookie in.  konst: c | C | the connector's metadata, zero-padded.
// After this c', kH and kV are of no further use: the lane wipes them from its slot.
__global__ __launch_bounds__(64) void k_con_initiate(uint8_t *__restrict__ out, uint8_t *x, const uint8_t *__restrict__ in,
                                                      uint8_t *__restrict__ state, const uint8_t *__restrict__ konst,
                                                      uint32_t meta_len, uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    u32 *o = words(out + (uint64_t)CZC_OUT2 * j);
    if (o[0] != CZA_ST_OK)
        return;
    const u32 *rec = words(in + (uint64_t)CZC_IN2 * j);
    u32 *st = words(state + (uint64_t)CZC_STATE * rec[CZC_IN2_SLOT / 4]);
    u32 *plain = words(x + (uint64_t)CZC_X2 * j + CZC_X2_PLAIN);
    const u32 *vn = rec + CZC_IN2_VNONCE / 4;
    {
        u32 d[16], vtag[4], kv[8];
        ldw(kv, st + CZC_STATE_KV / 4);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            d[i] = rec[CZC_IN2_CP / 4 + i];
            d[8 + i] = rec[CZC_IN2_SERVER / 4 + i];
        }
        const u32 n[6] = {w4('V', 'O', 'U', 'C'), w4('H', '-', '-', '-'), vn[0], vn[1], vn[2], vn[3]};
        xs_fixed<4, false>(d, vtag, kv, n);
#pragma unroll
        for (int i = 0; i < 8; i++)
            plain[i] = words(konst + CZC_KONST_PUBLIC)[i];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            plain[8 + i] = vn[i];
            plain[12 + i] = vtag[i];
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
            plain[16 + i] = d[i];
    }
    const u32 meta_words = (meta_len + 15u) / 16u * 4u;  // at most CZC_META_MAX / 4, checked by the host side
    for (u32 i = 0; i < meta_words; i++)
        plain[32 + i] = words(konst + CZC_KONST_META)[i];
    u32 pre[8], tag[4];
    ldw(pre, st + CZC_STATE_PRECOM / 4);
    const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('I', 'N', 'I', 'T'), w4('I', 'A', 'T', 'E'),
                      0u, 0x02000000u};
    u32 *box = o + (CZC_OUT2_CMD + 113) / 4;
    xs_mem<false>(plain, box + 4, 128u + meta_len, tag, pre, n);
    o[4] = w4('\0', '\0', '\0', '\x08');
    o[5] = w4('I', 'N', 'I', 'T');
    o[6] = w4('I', 'A', 'T', 'E');
    o[(CZC_OUT2_CMD + 105) / 4] = 0u;
    o[(CZC_OUT2_CMD + 105) / 4 + 1] = 0x02000000u;
#pragma unroll
    for (int i = 0; i < 4; i++)
        box[i] = tag[i];
    wipe_words(st + CZC_STATE_SECRET / 4, 16);
    wipe_words(st + CZC_STATE_KV / 4, 8);
}

// Stage 3, one lane per READY of a plausible size.  in: CZC_IN3 records; out: CZC_OUT3 records (status
// CZA_ST_NOT_RUN until a lane writes its own).  Opens Box [metadata](S'->C') under the slot's cnPrecom and
// nonce "CurveZMQREADY---" + the command's 8 bytes, and hands cnPrecom out with the plaintext.
__global__ __launch_bounds__(64) void k_con_ready(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                   const uint8_t *__restrict__ state, uint32_t count)
{
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count)
        return;
    const u32 *rec = words(in + (uint64_t)CZC_IN3 * j);
    u32 *o = words(out + (uint64_t)CZC_OUT3 * j);
    const u32 *st = words(state + (uint64_t)CZC_STATE * rec[CZC_IN3_SLOT / 4]);
    u32 pre[8], tin[4], tag[4];
    ldw(pre, st + CZC_STATE_PRECOM / 4);
    ldw(tin, rec + CZC_IN3_BOX / 4);
    const u32 nbytes = rec[CZC_IN3_LEN / 4];  // 0 .. CZC_READY_MAX, checked by the host side
    const u32 n[6] = {w4('C', 'u', 'r', 'v'), w4('e', 'Z', 'M', 'Q'), w4('R', 'E', 'A', 'D'), w4('Y', '-', '-', '-'),
                      rec[CZC_IN3_NONCE / 4], rec[CZC_IN3_NONCE / 4 + 1]};
    u32 *plain = o + CZC_OUT3_PLAIN / 4;
    xs_mem<true>(rec + CZC_IN3_BOX / 4 + 4, plain, nbytes, tag, pre, n);
    if (diff<4>(tag, tin)) {
        wipe_words(plain, (nbytes + 15u) / 16u * 4u);
        o[0] = CZA_ST_CRYPTO;
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        o[CZC_OUT3_PRECOM / 4 + i] = pre[i];
    o[0] = CZA_ST_OK;
}

}  // namespace

extern "C" {

hipError_t czk_con_hello(const void *in, const void *x, void *out, void *state, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_con_hello, count, s, in, x, out, state, count);
}

hipError_t czk_con_welcome(const void *in, void *out, void *x, const void *state, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_con_welcome, count, s, in, out, x, state, count);
}

hipError_t czk_con_initiate(void *out, void *x, const void *in, void *state, const void *konst, uint32_t meta_len,
                            uint32_t count, hipStream_t s)
{
    return launch_lanes(k_con_initiate, count, s, out, x, in, state, konst, meta_len, count);
}

hipError_t czk_con_ready(const void *in, void *out, const void *state, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_con_ready, count, s, in, out, state, count);
}

}  // extern "C"
