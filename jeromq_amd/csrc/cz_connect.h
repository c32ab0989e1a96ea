// cz_connect.h -- records shared by the batched client handshake's kernels (cz_connect_kernels.h) and
// its host side (cz_connector.cpp).  Every record is a multiple of 16 bytes and every field 4-byte
// aligned: the kernels read and write whole dwords.  Key agreements are cza_job lanes of k_x25519_jobs
// and the status words are the handshakes' common ones (cz_hs_records.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_hs_records.h"

// slot state record (device table, one per pending connection): every field is a secret
#define CZC_STATE 128
#define CZC_STATE_SECRET 0       // c', wiped once the INITIATE is made
#define CZC_STATE_KH 32          // kH = beforenm(S, c'): HELLO and WELCOME boxes, wiped with c'
#define CZC_STATE_PRECOM 64      // cnPrecom = beforenm(S', c')
#define CZC_STATE_KV 96          // kV = beforenm(S', c): the vouch's key, wiped with c'

// the connector's constants on the device: c | C | metadata padded with zeros to CZC_META_MAX
#define CZC_META_MAX 256
#define CZC_KONST (64 + CZC_META_MAX)
#define CZC_KONST_SECRET 0
#define CZC_KONST_PUBLIC 32
#define CZC_KONST_META 64

// stage 1 (hello) input, one per connection that got a slot
#define CZC_IN1 80
#define CZC_IN1_SERVER 0         // S
#define CZC_IN1_SECRET 32        // c'
#define CZC_IN1_SLOT 64
// stage 1 key agreements, one per record: C' = c'.9, kH
#define CZC_X1 64
// stage 1 output
#define CZC_OUT1 224
#define CZC_OUT1_STATUS 0
#define CZC_OUT1_CMD 16          // the 200-byte HELLO

// stage 2 (welcome) input, one per WELCOME of the right size on a slot that waits for it
#define CZC_IN2 256
#define CZC_IN2_SLOT 0
#define CZC_IN2_NONCE 16         // WELCOME bytes 8..24
#define CZC_IN2_BOX 32           // WELCOME bytes 24..168: tag 16, body 128 (S' 32, cookie 96)
#define CZC_IN2_SERVER 176       // S
#define CZC_IN2_CP 208           // C'
#define CZC_IN2_VNONCE 240       // the vouch nonce's 16 random bytes
// stage 2 device scratch, one per record: S' from the WELCOME box, then the INITIATE plaintext
#define CZC_INIT_MAX (128 + CZC_META_MAX)
#define CZC_X2 (32 + CZC_INIT_MAX)
#define CZC_X2_SP 0
#define CZC_X2_PLAIN 32          // C 32, vouch nonce 16, vouch box 80, metadata
// stage 2 output.  The INITIATE command starts 3 bytes into a word, so that its cookie (byte 9), nonce
// (105) and box (113) are dword-aligned for the kernels.
#define CZC_OUT2 544
#define CZC_OUT2_STATUS 0
#define CZC_OUT2_CMD 19          // "\x08INITIATE" | cookie 96 | nonce 8 | tag 16 | body up to CZC_INIT_MAX
#define CZC_INITIATE_MAX (113 + 16 + CZC_INIT_MAX)

// stage 3 (ready) input, one per READY of a plausible size on a slot that waits for it
#define CZC_READY_MAX 256        // READY plaintext (the server's metadata)
#define CZC_IN3 288
#define CZC_IN3_SLOT 0
#define CZC_IN3_LEN 4            // plaintext bytes
#define CZC_IN3_NONCE 8          // READY bytes 6..14
#define CZC_IN3_BOX 16           // READY bytes 14..: tag 16, body up to CZC_READY_MAX
// stage 3 output
#define CZC_OUT3 304
#define CZC_OUT3_STATUS 0
#define CZC_OUT3_PRECOM 16       // cnPrecom, for accepted lanes only
#define CZC_OUT3_PLAIN 48        // the READY plaintext

static_assert(CZC_OUT2_CMD + CZC_INITIATE_MAX <= CZC_OUT2, "the largest INITIATE fits its record");
static_assert((CZC_OUT2_CMD + 9) % 4 == 0 && (CZC_OUT2_CMD + 113) % 16 == 4, "INITIATE fields are dword-aligned");

extern "C" {
hipError_t czk_con_hello(const void *in, const void *x, void *out, void *state, uint32_t count, hipStream_t s);
hipError_t czk_con_welcome(const void *in, void *out, void *x, const void *state, uint32_t count, hipStream_t s);
hipError_t czk_con_initiate(void *out, void *x, const void *in, void *state, const void *konst, uint32_t meta_len,
                            uint32_t count, hipStream_t s);
hipError_t czk_con_ready(const void *in, void *out, const void *state, uint32_t count, hipStream_t s);
}
