// cz_wire.cpp -- ZMTP v2 framing: host parser (V2Decoder rules) and the device pack/unpack launcher.
//
// Reference: zmq/io/coder/v2/V2Encoder.java:31-55 (flags byte, 1-byte or BE64 size),
// V2Decoder.java:37-105 (flagsReady / oneByteSizeReady / eightByteSizeReady), and the size
// checks of zmq/io/coder/Decoder.java:76-98.  The parse of ONE stream is a sequential walk over one
// header per frame (the bodies are never touched here) and runs on the host, while the byte movement
// (packing sealed bodies behind their headers, unpacking received bodies into aligned slots)
// runs on the device in k_v2_copy.  MANY streams are as many independent walks: cz_v2_scan /
// cz_v2_scan_emit / cz_open_streams / cz_relay_streams run them on the device, one lane per stream, with the
// same rules.
#include <stdint.h>
#include <string.h>

#include "cz_internal.h"

using namespace czi;

extern "C" {

uint32_t cz_v2_header_size(uint64_t size) { return size > 255u ? 9u : 2u; }

int cz_v2_parse(const uint8_t *wire, uint64_t len, int64_t maxmsgsize, cz_v2_frame *frames, uint32_t cap,
                uint32_t *nframes, uint64_t *consumed)
{
    if (!nframes || !consumed || (len && !wire) || (cap && !frames))
        return fail(CZ_EINVAL, "cz_v2_parse: null pointer");
    uint64_t p = 0;
    uint32_t nf = 0;
    int rc = CZ_OK;
    while (nf < cap && p < len) {
        const uint8_t f = wire[p];
        uint64_t size, h;
        if (f & CZ_V2_LARGE) {
            if (len - p < 9)
                break;
            size = 0;
            for (int b = 1; b <= 8; b++)
                size = (size << 8) | wire[p + b];  // Wire.getUInt64: big-endian
            h = 9;
            if ((int64_t)size <= 0) {  // V2Decoder.eightByteSizeReady: `size <= 0` on a Java long
                rc = fail(CZ_EPROTO, "cz_v2_parse: 8-byte frame size %lld at offset %llu",
                          (long long)(int64_t)size, (unsigned long long)p);
                break;
            }
        } else {
            if (len - p < 2)
                break;
            size = wire[p + 1];
            h = 2;
        }
        // Decoder.sizeReady: maxmsgsize, then the int range of a Java array
        if ((maxmsgsize >= 0 && size > (uint64_t)maxmsgsize) || size > 0x7fffffffull) {
            rc = fail(CZ_EMSGSIZE, "cz_v2_parse: frame size %llu at offset %llu exceeds the limit",
                      (unsigned long long)size, (unsigned long long)p);
            break;
        }
        if (len - p - h < size)
            break;  // body not complete yet: keep the bytes for the next read
        uint32_t mf = 0;
        if (f & CZ_V2_MORE)
            mf |= CZ_MSG_MORE;
        if (f & CZ_V2_COMMAND)
            mf |= CZ_MSG_COMMAND;
        frames[nf++] = {p + h, (uint32_t)size, mf};
        p += h + size;
    }
    *nframes = nf;
    *consumed = p;
    return rc;
}

int cz_v2_copy(const cz_v2_item *d_items, uint32_t count, const void *d_src, void *d_dst, void *stream)
{
    if (count && (!d_items || !d_src || !d_dst))
        return fail(CZ_EINVAL, "cz_v2_copy: null pointer");
    hipError_t e = czk_v2_copy(d_items, count, d_src, d_dst, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : hip_fail(e, "cz_v2_copy");
}

static bool bad_slot_align(uint32_t a) { return a == 0 || a > 4096u || (a & (a - 1u)) != 0; }

int cz_v2_scan(const cz_v2_stream *d_streams, uint32_t count, const void *d_wire, int64_t maxmsgsize,
               uint32_t slot_align, cz_v2_stream_result *d_results, cz_v2_totals *d_totals, void *stream)
{
    if (!d_totals || (count && (!d_streams || !d_wire || !d_results)))
        return fail(CZ_EINVAL, "cz_v2_scan: null pointer");
    if (bad_slot_align(slot_align))
        return fail(CZ_EINVAL, "cz_v2_scan: slot_align %u is not a power of two from 1 to 4096", slot_align);
    hipError_t e = czk_v2_scan(d_streams, count, d_wire, maxmsgsize, slot_align, d_results, d_totals, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : hip_fail(e, "cz_v2_scan");
}

int cz_v2_scan_emit(const cz_v2_stream *d_streams, const cz_v2_stream_result *d_results, uint32_t count,
                    const void *d_wire, uint32_t slot_align, cz_v2_frame *d_frames, cz_frame_desc *d_desc, void *stream)
{
    if (count && (!d_streams || !d_wire || !d_results))
        return fail(CZ_EINVAL, "cz_v2_scan_emit: null pointer");
    if (bad_slot_align(slot_align))
        return fail(CZ_EINVAL, "cz_v2_scan_emit: slot_align %u is not a power of two from 1 to 4096", slot_align);
    hipError_t e = czk_v2_emit(d_streams, d_results, count, d_wire, slot_align, d_frames, d_desc, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : hip_fail(e, "cz_v2_scan_emit");
}

// the calling thread's device totals record of cz_open_streams, per device (never freed: at thread or
// process exit the runtime may be gone first)
static thread_local struct {
    DevBuf buf;
    int device = -1;
} t_totals;

// that record for the current device
static hipError_t thread_totals(cz_v2_totals **d_totals)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    if (dev != t_totals.device) {
        t_totals.buf = DevBuf{};
        t_totals.device = -1;
        if ((e = t_totals.buf.reserve(sizeof(cz_v2_totals))) != hipSuccess)
            return e;
        t_totals.device = dev;
    }
    *d_totals = (cz_v2_totals *)t_totals.buf.ptr;
    return hipSuccess;
}

int cz_open_streams(const cz_v2_stream *d_streams, uint32_t count, const void *d_wire, int64_t maxmsgsize,
                    uint32_t slot_align, cz_v2_stream_result *d_results, cz_frame_desc *d_desc, uint64_t desc_cap,
                    void *d_out, uint64_t out_cap, const void *d_subkeys, uint16_t *d_status, uint64_t *d_nonces,
                    cz_v2_totals *h_totals, void *stream)
{
    if (!h_totals || !d_subkeys || !d_status || (desc_cap && !d_desc) || (out_cap && !d_out) ||
        (count && (!d_streams || !d_wire || !d_results)))
        return fail(CZ_EINVAL, "cz_open_streams: null pointer");
    if (bad_slot_align(slot_align))
        return fail(CZ_EINVAL, "cz_open_streams: slot_align %u is not a power of two from 1 to 4096", slot_align);
    *h_totals = {0, 0};
    if (count == 0)
        return CZ_OK;
    hipStream_t s = (hipStream_t)stream;
    cz_v2_totals *d_totals = nullptr;
    hipError_t e = thread_totals(&d_totals);
    if (e != hipSuccess)
        return hip_fail(e, "cz_open_streams");
    if ((e = czk_v2_scan(d_streams, count, d_wire, maxmsgsize, slot_align, d_results, d_totals, s)) != hipSuccess ||
        (e = hipMemcpyAsync(h_totals, d_totals, sizeof *h_totals, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(e, "cz_open_streams: scan");
    if (h_totals->nframes > 0x7fffffffull)
        return fail(CZ_EINVAL, "cz_open_streams: %llu frames, more than 2^31 - 1", (unsigned long long)h_totals->nframes);
    if (h_totals->nframes > desc_cap || h_totals->slot_bytes > out_cap)
        return fail(CZ_ENOMEM, "cz_open_streams: %llu frames / %llu slot bytes exceed desc_cap %llu / out_cap %llu",
                    (unsigned long long)h_totals->nframes, (unsigned long long)h_totals->slot_bytes,
                    (unsigned long long)desc_cap, (unsigned long long)out_cap);
    if ((e = czk_v2_emit(d_streams, d_results, count, d_wire, slot_align, nullptr, d_desc, s)) != hipSuccess ||
        (e = czk_open_desc(d_desc, nullptr, (uint32_t)h_totals->nframes, d_wire, d_out, d_subkeys, d_status, d_nonces,
                           s)) != hipSuccess)
        return hip_fail(e, "cz_open_streams: open");
    return CZ_OK;
}

// Section 3j: cz_open_streams' chain with the relay in the open's place.  The emit materialises every frame's
// replay floor before the relay stores anything, so the bodies are re-sealed where they lie; the cut then says
// what of each stream may leave.
int cz_relay_streams(const cz_v2_stream *d_streams, const cz_fanout_sub *d_to, uint32_t count, const void *d_wire,
                     void *d_out, int64_t maxmsgsize, cz_v2_stream_result *d_scan, cz_frame_desc *d_desc,
                     cz_fanout_sub *d_to_frames, uint64_t desc_cap, const void *d_subkeys, uint16_t *d_status,
                     uint64_t *d_nonces, cz_relay_stream_result *d_results, cz_v2_totals *h_totals, void *stream)
{
    if (!h_totals)
        return fail(CZ_EINVAL, "cz_relay_streams: null pointer");
    *h_totals = {0, 0};
    if (count == 0)
        return CZ_OK;
    if (!d_streams || !d_to || !d_wire || !d_out || !d_scan || !d_desc || !d_to_frames || !d_subkeys || !d_status ||
        !d_nonces || !d_results)
        return fail(CZ_EINVAL, "cz_relay_streams: null pointer");
    hipStream_t s = (hipStream_t)stream;
    cz_v2_totals *d_totals = nullptr;
    hipError_t e = thread_totals(&d_totals);
    if (e != hipSuccess)
        return hip_fail(e, "cz_relay_streams");
    if ((e = czk_v2_scan(d_streams, count, d_wire, maxmsgsize, 1u, d_scan, d_totals, s)) != hipSuccess ||
        (e = hipMemcpyAsync(h_totals, d_totals, sizeof *h_totals, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(e, "cz_relay_streams: scan");
    if (h_totals->nframes > 0x7fffffffull)
        return fail(CZ_EINVAL, "cz_relay_streams: %llu frames, more than 2^31 - 1", (unsigned long long)h_totals->nframes);
    if (h_totals->nframes > desc_cap)
        return fail(CZ_ENOMEM, "cz_relay_streams: %llu frames exceed desc_cap %llu",
                    (unsigned long long)h_totals->nframes, (unsigned long long)desc_cap);
    if ((e = czk_v2_emit_relay(d_streams, d_to, d_scan, count, d_wire, d_out, d_desc, d_to_frames, s)) != hipSuccess ||
        (e = czk_relay_desc(d_desc, d_to_frames, nullptr, (uint32_t)h_totals->nframes, d_wire, d_out, d_subkeys,
                            d_status, d_nonces, s)) != hipSuccess ||
        (e = czk_relay_cut(d_streams, d_scan, count, d_desc, d_status, d_nonces, d_results, s)) != hipSuccess)
        return hip_fail(e, "cz_relay_streams: relay");
    return CZ_OK;
}

}  // extern "C"
