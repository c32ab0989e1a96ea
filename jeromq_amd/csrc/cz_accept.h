// cz_accept.h -- records shared by the batched server handshake's kernels (cz_accept_kernels.h) and its
// host side (cz_acceptor.cpp).  Every record is a multiple of 16 bytes and every field 4-byte
// aligned: the kernels read and write whole dwords.  Key agreements are cza_job lanes of k_x25519_jobs
// and the status words are the handshakes' common ones (cz_hs_records.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cz_hs_records.h"

// slot state record (device table, one per pending connection): every field is a secret or binds one
#define CZA_STATE 128
#define CZA_STATE_SECRET 0       // s'
#define CZA_STATE_COOKIE_KEY 32
#define CZA_STATE_PRECOM 64      // cnPrecom = beforenm(C', s')
#define CZA_STATE_CP 96          // C'

// stage 1 input, one per well-formed HELLO
#define CZA_IN1 240
#define CZA_IN1_CP 0             // C' (HELLO bytes 80..112)
#define CZA_IN1_NONCE 32         // HELLO bytes 112..120
#define CZA_IN1_BOX 48           // HELLO bytes 120..200: tag 16, body 64
#define CZA_IN1_ENTROPY 128      // cookie nonce 16, cookie key 32, WELCOME nonce 16
#define CZA_IN1_SECRET 192       // s'
#define CZA_IN1_SLOT 224
// stage 1 key agreements, one per record: S', k1, cnPrecom
#define CZA_X1 96
// stage 1 output
#define CZA_OUT1 192
#define CZA_OUT1_STATUS 0
#define CZA_OUT1_CMD 16          // the 168-byte WELCOME

// stage 2 input, one per INITIATE of a plausible size
#define CZA_INIT_MAX 384         // INITIATE plaintext: 128 + at most 256 bytes of metadata
#define CZA_IN2 544
#define CZA_IN2_SLOT 0
#define CZA_IN2_LEN 4            // plaintext bytes (box body)
#define CZA_IN2_NONCE 8          // INITIATE bytes 105..113
#define CZA_IN2_COOKIE_NONCE 16  // INITIATE bytes 9..25
#define CZA_IN2_COOKIE 32        // INITIATE bytes 25..105: tag 16, body 64
#define CZA_IN2_BOX 128          // INITIATE bytes 113..: tag 16, body up to CZA_INIT_MAX
// stage 2 output
#define CZA_META_MAX 256
#define CZA_OUT2 704
#define CZA_OUT2_STATUS 0
#define CZA_OUT2_PRECOM 16       // cnPrecom, for accepted lanes only
#define CZA_OUT2_READY 48        // READY box: tag 16, body up to CZA_META_MAX
#define CZA_OUT2_PLAIN 320       // INITIATE plaintext: C 32, vouch nonce 16, vouch box 80, metadata

extern "C" {
hipError_t czk_acc_welcome(const void *in, const void *x, void *out, void *state, uint32_t count, hipStream_t s);
hipError_t czk_acc_initiate(const void *in, void *out, const void *state, uint32_t count, hipStream_t s);
hipError_t czk_acc_ready(void *out, const void *x, const void *in, const void *state, const void *meta,
                         uint32_t meta_len, uint32_t count, hipStream_t s);
}
