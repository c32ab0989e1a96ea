// cz_hs_dev.h -- device helpers of the batched CURVE handshakes that belong to neither side: the
// register and memory forms of the NaCl box (xs_fixed, xs_mem), the dword helpers around them, the
// per-lane-job X25519 kernel and the launch wrapper every handshake kernel goes through.  Compiled as
// part of cz_x25519.hip, the handshake's device translation unit: k_x25519_jobs here and k_x25519 there
// run the same ladder (cz_fe25519.h), and the library keeps one code object for both.  The server's
// kernels are in cz_accept_kernels.h, the client's in cz_connect_kernels.h.
//
// NaCl's rules as in k_nacl_one: a seal keys Poly1305 with c[0:32] (the keystream here: these boxes'
// m[0:32] is zero), an open with the keystream; tags are compared without an early exit; a failed
// open leaves no plaintext behind.  A lane whose check fails writes its status and returns; its
// neighbours in the wave carry on.  The boxes are 96 to 416 bytes: every lane reads and writes its
// own 4-byte-aligned records with dword accesses, no line staging.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_fe25519.h"
#include "cz_hs_records.h"

namespace {

using cz::hsalsa20;
using cz::Poly;
using cz::poly_block;
using cz::poly_block_partial;
using cz::poly_finish;
using cz::poly_init;
using cz::salsa20_block;

// four ASCII characters as the little-endian word a dword load of them gives
constexpr u32 w4(char a, char b, char c, char d)
{
    return (u32)(uint8_t)a | ((u32)(uint8_t)b << 8) | ((u32)(uint8_t)c << 16) | ((u32)(uint8_t)d << 24);
}

__device__ __forceinline__ const u32 *words(const uint8_t *p) { return reinterpret_cast<const u32 *>(p); }
__device__ __forceinline__ u32 *words(uint8_t *p) { return reinterpret_cast<u32 *>(p); }

template <int N>
__device__ __forceinline__ void ldw(u32 (&o)[N], const u32 *p)
{
#pragma unroll
    for (int i = 0; i < N; i++)
        o[i] = p[i];
}

// 0 iff a[0:N) == b[0:N), every word looked at
template <int N>
__device__ __forceinline__ u32 diff(const u32 *a, const u32 *b)
{
    u32 d = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
        d |= a[i] ^ b[i];
    return d;
}

// XSalsa20-Poly1305 over NCH 16-byte chunks held in registers, in place: d = m[32:] (seal) or
// c[32:] (open) on entry, the other on return; tag = Poly1305 of the ciphertext.  n = the 24-byte
// nonce as words.  The box's first 32 bytes are zero, so keystream bytes [0,32) are the MAC key and
// chunk j takes keystream bytes [32 + 16j, 48 + 16j).
template <int NCH, bool OPEN>
__device__ __forceinline__ void xs_fixed(u32 (&d)[4 * NCH], u32 tag[4], const u32 key[8], const u32 n[6])
{
    u32 sub[8];
    const u32 in4[4] = {n[0], n[1], n[2], n[3]};
    hsalsa20(sub, key, in4);
    Poly P;
    constexpr int NB = (32 + 16 * NCH + 63) / 64;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        u32 x[16];
        salsa20_block<false>(x, sub, n[4], n[5], (u32)b, 0u);
        if (b == 0)
            poly_init(P, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = 4 * b + c - 2;
            if (j < 0 || j >= NCH)
                continue;
            if (OPEN)
                poly_block(P, d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3], 1u);
#pragma unroll
            for (int k = 0; k < 4; k++)
                d[4 * j + k] ^= x[4 * c + k];
            if (!OPEN)
                poly_block(P, d[4 * j], d[4 * j + 1], d[4 * j + 2], d[4 * j + 3], 1u);
        }
    }
    poly_finish(P, tag);
}

// the first cnt bytes (1..16) of a 16-byte chunk, the rest cleared
__device__ __forceinline__ void keep_bytes(u32 v[4], u32 cnt)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int rel = (int)cnt - 4 * i;
        v[i] &= rel >= 4 ? 0xffffffffu : (rel <= 0 ? 0u : ((1u << (8 * rel)) - 1u));
    }
}

// The same over nbytes (1..CZA_INIT_MAX) in memory: in -> out, both 4-byte aligned and padded to
// whole 16-byte chunks (the pad bytes of out are written as zero).
template <bool OPEN>
__device__ __forceinline__ void xs_mem(const u32 *__restrict__ in, u32 *__restrict__ out, u32 nbytes, u32 tag[4],
                                       const u32 key[8], const u32 n[6])
{
    u32 sub[8];
    const u32 in4[4] = {n[0], n[1], n[2], n[3]};
    hsalsa20(sub, key, in4);
    Poly P;
    poly_init(P, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u);
    const u32 end = 32u + nbytes;
    const u32 nblk = (end + 63u) >> 6;
    for (u32 b = 0; b < nblk; b++) {
        u32 x[16];
        salsa20_block<false>(x, sub, n[4], n[5], b, 0u);
        if (b == 0)
            poly_init(P, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const u32 oc = 64u * b + 16u * (u32)c;
            if (oc < 32u || oc >= end)
                continue;
            const u32 cnt = end - oc < 16u ? end - oc : 16u;
            const u32 w = (oc - 32u) >> 2;
            u32 v[4] = {in[w], in[w + 1], in[w + 2], in[w + 3]};
            if (OPEN) {
                if (cnt == 16u)
                    poly_block(P, v[0], v[1], v[2], v[3], 1u);
                else
                    poly_block_partial(P, v[0], v[1], v[2], v[3], cnt);
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                v[k] ^= x[4 * c + k];
            keep_bytes(v, cnt);
            if (!OPEN) {
                if (cnt == 16u)
                    poly_block(P, v[0], v[1], v[2], v[3], 1u);
                else
                    poly_block_partial(P, v[0], v[1], v[2], v[3], cnt);
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                out[w + k] = v[k];
        }
    }
    poly_finish(P, tag);
}

__device__ __forceinline__ void wipe_words(u32 *p, u32 nwords)
{
    for (u32 i = 0; i < nwords; i++)
        p[i] = 0u;
}

// One lane per key agreement, each lane its own job: out = X25519(scalar, point) (point = 9 with
// CZA_JOB_BASE), through NaCl's beforenm HSalsa20 with CZA_JOB_BEFORENM.  A job with a gate runs
// only if the gate word (a status an earlier kernel of the stage wrote) is zero.
__global__ __launch_bounds__(64) void k_x25519_jobs(const cza_job *__restrict__ jobs, uint32_t count)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count)
        return;
    const cza_job jb = jobs[i];
    if (jb.gate && *jb.gate != 0u)
        return;
    u32 k[8], u[8], r[8];
    load_words(k, jb.scalar);
    if (jb.flags & CZA_JOB_BASE) {
#pragma unroll
        for (int w = 0; w < 8; w++)
            u[w] = w == 0 ? 9u : 0u;
    } else {
        load_words(u, jb.point);
    }
    x25519(r, k, u);
    if (jb.flags & CZA_JOB_BEFORENM) {
        u32 o[8];
        const u32 zero[4] = {0u, 0u, 0u, 0u};
        hsalsa20(o, r, zero);
        store_words(jb.out, o);
    } else {
        store_words(jb.out, r);
    }
}

// How every handshake kernel is launched: one lane per item in blocks of 64, nothing for an empty
// batch.  The C wrappers' void pointers are cast to the kernel's parameter types here.
template <class... P, class... A>
hipError_t launch_lanes(void (*kernel)(P...), uint32_t count, hipStream_t s, A... args)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((count + 63) / 64), dim3(64), 0, s, (P)args...);
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t czk_x25519_jobs(const cza_job *jobs, uint32_t count, hipStream_t s)
{
    return launch_lanes(k_x25519_jobs, count, s, jobs, count);
}
