// cz_x25519.hip -- X25519 and NaCl crypto_box_beforenm on gfx950 (the CURVE handshake's key agreement).
//
// Reference: Curve.beforenm / keypair / box / open (jeromq-core/.../curve/Curve.java:100-193) call
// jnacl's curve25519xsalsa20poly1305.crypto_box_{beforenm,keypair,,_open}; a CURVE handshake runs
// two beforenm per side (HELLO/WELCOME boxes use C'/S', INITIATE's vouch uses C/S':
// CurveClientMechanism.java:246-419, CurveServerMechanism.java:254-507), and the MESSAGE key
// cnPrecom = beforenm(peer', our') (CurveClientMechanism.java:310).
//
// Algorithm: RFC 7748 section 5 -- clamped scalar, u masked to 255 bits, Montgomery ladder with
// a24 = 121665 and constant-time (masked) swaps, then x2 * z2^(p-2).  One lane per scalar
// multiplication: each lane's ladder is 255 serial steps of ~10 field multiplications, so a
// batch of independent key agreements (connection churn) fills the chip with no cross-lane work.
//
// Field arithmetic mod p = 2^255 - 19 in radix 2^25.5: 10 u32 limbs of 26/25 bits (limb i at bit
// ceil(25.5 i)).  A product is 100 v_mad_u64_u32 into u64 column sums; an odd*odd limb pair gains
// a factor 2 and a column >= 10 wraps with factor 19 (2^255 = 19 mod p).  Inputs to mul are kept
// below 2^27 per limb, so 19*g < 2^32 and each column stays below 2^63.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_fe25519.h"
#include "cz_hs_dev.h"  // the batched handshakes' box helpers and k_x25519_jobs: the same ladder, one code object
#include "cz_accept_kernels.h"   // the batched server handshake's kernels
#include "cz_connect_kernels.h"  // the batched client handshake's

namespace {

// one lane per key agreement: out = X25519(scalar, point), point = 9 when points == nullptr
__global__ __launch_bounds__(64) void k_x25519(const uint8_t *__restrict__ scalars, const uint8_t *__restrict__ points,
                                                uint8_t *__restrict__ out, uint32_t count, int beforenm)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count)
        return;
    u32 k[8], u[8], r[8];
    load_words(k, scalars + 32ull * i);
    if (points) {
        load_words(u, points + 32ull * i);
    } else {
#pragma unroll
        for (int w = 0; w < 8; w++)
            u[w] = w == 0 ? 9u : 0u;
    }
    x25519(r, k, u);
    if (beforenm) {
        // NaCl crypto_box_beforenm: HSalsa20(shared, 0^16) with the "expand 32-byte k" constants
        u32 o[8];
        const u32 zero[4] = {0u, 0u, 0u, 0u};
        cz::hsalsa20(o, r, zero);
        store_words(out + 32ull * i, o);
    } else {
        store_words(out + 32ull * i, r);
    }
}

}  // namespace

extern "C" hipError_t czk_x25519(const void *scalars, const void *points, void *out, uint32_t count, int beforenm,
                                 hipStream_t s)
{
    return launch_lanes(k_x25519, count, s, scalars, points, out, count, beforenm);
}
