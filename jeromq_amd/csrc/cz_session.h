// cz_session.h -- bulk session hand-over (section 13 of the header): what the kernels, the engine and the
// two batched handshakes share.  Not part of the C-ABI.
//
// One job record per session; k_session_subkeys runs two lanes on it (tx and rx).  The key is read from
// `base + src_off`: base is the handshake's device state (src_off = slot * 128 + 64, the record's
// cnPrecom) or the engine's staged array of precoms (src_off = 32 * j), both 32-byte aligned.  tx_key
// and rx_key index the engine's subkey table; a reused connection id keeps its old key slots, so they
// are per job, never derived from the lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct cz_session_job {
    uint64_t src_off;  // bytes from the base pointer to the session's 32-byte cnPrecom, a multiple of 32
    uint32_t tx_key;   // subkey table index of the key this side seals under
    uint32_t rx_key;   // ... and of the key it opens under
    uint32_t server;   // 1: the CurveServerMechanism side (tx = MESSAGES, rx = MESSAGEC), 0: the client
    uint32_t reserved;
};
static_assert(sizeof(cz_session_job) == 24, "cz_session_job layout");

// (the launchers czk_session_subkeys and czk_scatter_wipe: cz_launch.h)

struct cz_engine;

namespace czi {

// One session of a bulk add.  ok == 0: a per-item failure found by the caller (ids[i] = CZ_EINVAL, no
// id consumed).  The key is at d_base + src_off when the call has a device base, else at h_key.
struct SessionItem {
    uint8_t ok, server;
    uint64_t src_off;
    const uint8_t *h_key;
    uint64_t nonce, peer_nonce;
};

int engine_device(const cz_engine *e);
// cz_engine_add_conn for items[0, count) in one device chain (cz_engine.cpp).  d_base: the device memory
// every item's src_off counts from, on the engine's device, or nullptr to stage the h_key's.
int engine_add_sessions(cz_engine *e, const char *where, uint32_t count, const SessionItem *items, const void *d_base,
                        int32_t *ids);

}  // namespace czi
