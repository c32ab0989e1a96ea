// cz_hs_records.h -- what the two batched handshakes (cz_acceptor, cz_connector) share on both sides of
// the launch: the key-agreement job record of k_x25519_jobs and the per-lane status words.  The records
// of each side's own stages are in cz_accept.h and cz_connect.h, which include this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one key agreement: out = X25519(scalar, point | 9) [-> HSalsa20(., 0^16)]; device addresses
struct cza_job {
    const uint8_t *scalar;
    const uint8_t *point;   // unused with CZA_JOB_BASE
    uint8_t *out;
    const uint32_t *gate;   // NULL, or a status word: the job runs only if it is CZA_ST_OK
    uint32_t flags;
    uint32_t pad;
};
#define CZA_JOB_BASE 1u
#define CZA_JOB_BEFORENM 2u

// per-lane status words
#define CZA_ST_OK 0u
#define CZA_ST_CRYPTO 1u        // a box or the cookie did not open / the cookie is another connection's
#define CZA_ST_KEY_EXCHANGE 3u  // the vouch names another short-term key
#define CZA_ST_NOT_RUN 0xffffffffu

extern "C" hipError_t czk_x25519_jobs(const cza_job *jobs, uint32_t count, hipStream_t s);
