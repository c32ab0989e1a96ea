// The case grid of tools/dispatch_record.py: calls the launchers of cz_kernels.hip (compiled host-only
// under shim.h, so they print instead of launching) with made-up addresses over the layouts at which
// a launcher's decision can change.  Prints one line per case, then the launches it made.
// The declarations are the driver's own: it has to build against any revision of csrc/.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "curvezmq_mi355x.h"

extern "C" {
hipError_t czk_seal_uniform(const void *, uint64_t, void *, uint64_t, uint32_t, uint32_t, const void *, uint64_t,
                            const uint8_t *, hipStream_t);
hipError_t czk_seal_uniform_box(const void *, uint64_t, void *, uint64_t, uint32_t, uint32_t, const void *, uint64_t,
                                hipStream_t);
hipError_t czk_open_uniform(const void *, uint64_t, void *, uint64_t, uint32_t, uint32_t, const void *, uint64_t, int,
                            uint16_t *, hipStream_t);
hipError_t czk_seal_fanout(const void *, uint32_t, uint32_t, const cz_fanout_sub *, const void *, void *, uint64_t,
                           uint32_t, hipStream_t);
int czk_fanout_class(uint64_t, uint32_t, uint32_t, int);
int czk_owns_slots(uint64_t);
hipError_t czk_seal_fanout_runs(const cz_fanout_run *, const cz_fanout_wave *, const uint32_t *, uint32_t, const void *,
                                const cz_fanout_sub *, const void *, void *, hipStream_t);
hipError_t czk_seal_segments(const cz_frame_desc *, const cz_segment *, uint32_t, const cz_combine *, uint32_t,
                             const void *, void *, const void *, void *, hipStream_t);
hipError_t czk_open_segments(const cz_frame_desc *, const cz_segment *, uint32_t, const cz_combine *, uint32_t,
                             const void *, void *, const void *, void *, uint16_t *, uint64_t *, hipStream_t);
int czk_tune(const char *, int);
// (weak: a revision of csrc/ from before the relay still links, and records no relay case)
hipError_t czk_relay_uniform(const void *, uint64_t, void *, uint64_t, uint32_t, uint32_t, const void *, uint64_t, int,
                             const void *, uint64_t, uint16_t *, hipStream_t) __attribute__((weak));
// (weak for the same reason: a revision from before the segmented relay records no relay_segments case)
hipError_t czk_relay_segments(const cz_frame_desc *, const cz_fanout_sub *, const cz_segment *, uint32_t,
                              const cz_combine *, uint32_t, uint32_t, const void *, void *, const void *, void *,
                              uint16_t *, uint64_t *, hipStream_t) __attribute__((weak));
}

namespace {

// made-up device buffers (shim.h prints a pointer as its buffer's letter + offset); nothing is ever dereferenced
const uint64_t IN = 1ull << 40, OUT = 2ull << 40, KEY = 3ull << 40, AUX = 4ull << 40;
const uint32_t SHIFT_TOTAL_MAX = (1u << 28) - 128u;
const uint32_t COUNTS[] = {1, 63, 64, 65, 1000, 1024, 1025, 1u << 20};
const uint32_t LENS[] = {0, 31, 32, 33, 63, 64, 222, 223, 4096, SHIFT_TOTAL_MAX - 33u, SHIFT_TOTAL_MAX - 32u};
const uint64_t PHASES[] = {0, 8, 1};  // a base on 16 bytes, on 8, odd
typedef std::vector<uint64_t> Strides;

template <class T>
T *ptr(uint64_t a)
{
    return reinterpret_cast<T *>(a);
}

struct Knob {
    const char *key;
    int value;
};
// the defaults, every knob off in turn, and open_carry = 2
const Knob KNOBS[] = {{nullptr, 0},    {"pair", 0},     {"un0", 0},        {"seglines", 0}, {"shift", 0},
                      {"open_ina", 0}, {"seal_ina", 0}, {"open_carry", 0}, {"shift16", 0},  {"open_carry", 2}};

struct WithKnob {
    const Knob &k;
    int old = 0;
    explicit WithKnob(const Knob &knob) : k(knob)
    {
        std::printf("knob %s=%d\n", k.key ? k.key : "default", k.value);
        if (k.key)
            old = czk_tune(k.key, k.value);
    }
    ~WithKnob()
    {
        if (k.key)
            czk_tune(k.key, old);
    }
};

void layout(const char *what, uint64_t ib, uint64_t is, uint64_t ob, uint64_t os, uint32_t n, uint32_t len)
{
    std::printf("%s %llu/%llu %llu/%llu n=%u len=%u\n", what, (unsigned long long)ib, (unsigned long long)is,
                (unsigned long long)ob, (unsigned long long)os, n, len);
}
void result(int rc)
{
    if (rc)
        std::printf("  rc=%d\n", rc);
}

// <what> <input base offset>/<stride> <output base offset>/<stride> n=<count> len=<len or size>
void seal(uint64_t ib, uint64_t is, uint64_t ob, uint64_t os, uint32_t n, uint32_t len)
{
    layout("seal", ib, is, ob, os, n, len);
    result(czk_seal_uniform(ptr<void>(IN + ib), is, ptr<void>(OUT + ob), os, n, len, ptr<void>(KEY), 7, ptr<uint8_t>(AUX),
                            nullptr));
}

void box(uint64_t ib, uint64_t is, uint64_t ob, uint64_t os, uint32_t n, uint32_t len)
{
    layout("box", ib, is, ob, os, n, len);
    result(czk_seal_uniform_box(ptr<void>(IN + ib), is, ptr<void>(OUT + ob), os, n, len, ptr<void>(KEY), 7, nullptr));
}

void open(uint64_t ib, uint64_t is, uint64_t ob, uint64_t os, uint32_t n, uint32_t size)
{
    layout("open", ib, is, ob, os, n, size);
    result(czk_open_uniform(ptr<void>(IN + ib), is, ptr<void>(OUT + ob), os, n, size, ptr<void>(KEY), 5, 1,
                            ptr<uint16_t>(AUX), nullptr));
}

// (one payload: no input stride; with czk_fanout_class's and czk_owns_slots' answers)
void fanout(uint64_t pb, uint64_t, uint64_t ob, uint64_t os, uint32_t n, uint32_t len)
{
    layout("fanout", pb, 0, ob, os, n, len);
    std::printf("  class=%d owns=%d\n", czk_fanout_class(os, len, n, ((pb | ob | os) & 15u) == 0), czk_owns_slots(os));
    result(czk_seal_fanout(ptr<void>(IN + pb), len, 1, ptr<cz_fanout_sub>(AUX), ptr<void>(KEY), ptr<void>(OUT + ob), os, n,
                           nullptr));
}
typedef void (*Call)(uint64_t, uint64_t, uint64_t, uint64_t, uint32_t, uint32_t);

// Output strides for `bytes` output bytes per slot: the bytes themselves, the 4 KiB and 100-byte
// layouts of the tests, the 256-slot region edge (64 * stride = 16384) and the next multiple of 16,
// the shifted stager's and the line stager's stride limits and the strides below them.  Below 64
// payload bytes only the first few: no stager's choice depends on more there.
Strides strides_for(uint32_t bytes, bool few)
{
    const Strides all = {bytes, 100, 112, 133, 144, 256, 272, 4224, 4097, 4104, 4129, 4136, (1ull << 22) - 16,
                         (1ull << 22) - 1, 1ull << 22, (1ull << 25) - 128, (1ull << 25) - 1, 1ull << 25};
    Strides v;
    for (uint64_t s : all)
        if (s >= bytes)
            v.push_back(s);
    if (bytes > (1u << 26))  // (no listed stride holds SHIFT_TOTAL_MAX bytes: one of each stager's)
        v = {4129, 4224, (1ull << 22) - 16, 1ull << 22};
    if (few && v.size() > 6)
        v.resize(6);
    return v;
}

// base and stride phases of input and output, independently: every input against four outputs (on
// a line, on 16 bytes, on 8, odd), every output against three inputs
void phase_cases(Call run, const Strides &in, const Strides &out, uint32_t len)
{
    for (uint64_t ib : PHASES)
        for (uint64_t is : in)
            for (uint64_t os : out)
                run(ib, is, 0, os, 1000, len);
    for (uint64_t ob : {8, 1})
        for (uint64_t os : out)
            for (uint64_t is : in)
                run(0, is, ob, os, 1000, len);
}

// output strides x lengths (extra = 33: an open's size for the seal's length), from an input that is
// aligned and one that is odd; at the lengths where a stager changes also 8-aligned, and to an odd output base
void length_cases(Call run, uint32_t extra)
{
    for (uint32_t len : LENS)
        for (uint64_t os : strides_for(extra ? len : len + 33u, len < 64))
            for (int lay = 0; lay < (len == 223 || len == 4096 ? 4 : 2); lay++) {
                const uint64_t ib = lay == 1 ? 1 : lay == 2 ? 8 : 0, ob = lay == 3 ? 1 : 0;
                run(ib, ((len + extra + 15u) & ~15ull) + 16 + ib, ob, os, 1000, len + extra);
            }
}

void knob_cases(Call run, uint32_t extra)
{
    for (uint64_t ib : PHASES) {
        const uint64_t is = (extra ? 4144u : 4096u) + ib;
        for (uint64_t os : {4224u, 4144u, 4129u})
            run(ib, is, 0, os, 1025, 4096 + extra);
        run(ib, 144 + ib, 0, 144, 1025, 100 + extra);
    }
    run(0, (extra ? 4144u : 4096u), 1, 4224, 1025, 4096 + extra);
    run(0, 144, 0, 133, 1025, 100 + extra);
}

void seal_cases()
{
    phase_cases(seal, {4096, 4104, 4097}, {4224, 4144, 4136, 4129}, 4000);
    phase_cases(seal, {112, 104, 101}, {256, 133}, 60);
    length_cases(seal, 0);
    for (uint32_t n : COUNTS) {
        seal(0, 4096, 0, 4224, n, 4096);
        seal(1, 4097, 0, 4224, n, 4096);
        seal(0, 4096, 1, 4129, n, 4096);
        seal(0, 112, 0, 144, n, 100);
    }
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        knob_cases(seal, 0);
    }
}

void open_cases()
{
    phase_cases(open, {4224, 4144, 4136, 4129}, {4096, 4112, 4104, 4097}, 4033);
    phase_cases(open, {256, 136, 133}, {256, 101}, 93);
    length_cases(open, 33);
    // bodies shorter than a MESSAGE's 33 bytes, and the body (not the plaintext) at SHIFT_TOTAL_MAX
    for (uint32_t size : {1u, 20u, 32u, SHIFT_TOTAL_MAX, SHIFT_TOTAL_MAX + 1u})
        for (uint64_t os : {144u, 256u, 4224u, 4129u})
            open(0, size + 16 - size % 16, 0, os, 1000, size);
    // 1024 = 64 P frames at in_stride 4136 (P = 16): the carried open with no block, with blocks
    // only, with blocks and a tail
    for (uint32_t n : COUNTS) {
        open(8, 4136, 0, 4096, n, 4129);
        open(0, 4144, 0, 4224, n, 4129);
        open(1, 4129, 0, 4096, n, 4129);
        open(0, 144, 0, 112, n, 133);
    }
    for (uint64_t os : {(1ull << 21) - 128, 1ull << 21})  // the carried open's offset limit: 64 P out_stride < 2^31
        open(8, 4136, 0, os, 2048, 4129);
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        knob_cases(open, 33);
        for (uint32_t n : {1000u, 1025u, 8193u}) {  // (P = 128 at in_stride 4129: blocks of 8192)
            open(8, 4136, 0, 4096, n, 4129);
            open(1, 4129, 0, 4096, n, 4129);
        }
    }
}

void box_cases()
{
    phase_cases(box, {4224, 4136, 4129}, {4224, 4144, 4136, 4129}, 4000);
    for (uint32_t len : LENS)
        for (uint64_t os : strides_for(len + 33u, len < 64))
            box(0, (len + 33u + 127u) & ~127ull, 0, os, 1000, len);
    for (uint32_t n : COUNTS) {
        box(0, 4224, 0, 4224, n, 4096);
        box(0, 144, 0, 144, n, 100);
    }
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        box(0, 4224, 0, 4224, 1025, 4096);
        box(0, 4224, 0, 4129, 1025, 4096);
        box(0, 144, 0, 144, 1025, 100);
    }
}

void fanout_cases()
{
    phase_cases(fanout, {0}, {4224, 4144, 4136, 4129}, 4000);
    phase_cases(fanout, {0}, {256, 144, 136, 133}, 60);
    for (uint32_t len : LENS)
        for (uint64_t os : strides_for(len + 33u, len < 64))
            fanout(0, 0, 0, os, 1000, len);
    for (uint32_t n : COUNTS)
        for (uint64_t os : {4224u, 4129u, 144u, 133u})
            fanout(0, 0, 0, os, n, os > 1000 ? 4096 : 100);
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        fanout(0, 0, 0, 4224, 1025, 4096);
        fanout(0, 0, 0, 4129, 1025, 4096);
        fanout(0, 0, 0, 144, 1025, 100);
    }
}

// grouped fan-out: class counts zero and non-zero per class; the region slice's stride 0, below, at
// and above REGION_MAX / 64
void fanout_runs_cases()
{
    for (int mask = 0; mask < 8; mask++)
        for (uint32_t rs : {0u, 100u, 256u, 257u}) {
            const uint32_t cc[3] = {mask & 1 ? 5u : 0u, mask & 2 ? 7u : 0u, mask & 4 ? 1025u : 0u};
            std::printf("fanout_runs classes=%u,%u,%u region_stride=%u\n", cc[0], cc[1], cc[2], rs);
            result(czk_seal_fanout_runs(ptr<cz_fanout_run>(AUX), ptr<cz_fanout_wave>(AUX + 4096), cc, rs, ptr<void>(IN),
                                        ptr<cz_fanout_sub>(AUX + 8192), ptr<void>(KEY), ptr<void>(OUT), nullptr));
        }
}

void segment_cases()
{
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        for (uint32_t nseg : {0u, 1u, 1025u})
            for (uint32_t ncomb : {0u, 1u}) {
                std::printf("seal_segments nseg=%u ncomb=%u\n", nseg, ncomb);
                result(czk_seal_segments(ptr<cz_frame_desc>(AUX), ptr<cz_segment>(AUX + 4096), nseg,
                                         ptr<cz_combine>(AUX + 8192), ncomb, ptr<void>(IN), ptr<void>(OUT), ptr<void>(KEY),
                                         ptr<void>(AUX + 12288), nullptr));
                std::printf("open_segments nseg=%u ncomb=%u\n", nseg, ncomb);
                result(czk_open_segments(ptr<cz_frame_desc>(AUX), ptr<cz_segment>(AUX + 4096), nseg,
                                         ptr<cz_combine>(AUX + 8192), ncomb, ptr<void>(IN), ptr<void>(OUT), ptr<void>(KEY),
                                         ptr<void>(AUX + 12288), ptr<uint16_t>(AUX + 16384), ptr<uint64_t>(AUX + 20480),
                                         nullptr));
            }
    }
}

// The relay's grid (`dispatch_record.py --relay`; not part of the default record): base and stride
// phases of input and output, the line emitter's stride and size limits, counts around a wave, every knob
void relay(uint64_t ib, uint64_t is, uint64_t ob, uint64_t os, uint32_t n, uint32_t size)
{
    layout("relay", ib, is, ob, os, n, size);
    result(czk_relay_uniform(ptr<void>(IN + ib), is, ptr<void>(OUT + ob), os, n, size, ptr<void>(KEY), 5, 1,
                             ptr<void>(KEY + 32), 9, ptr<uint16_t>(AUX), nullptr));
}

void relay_cases()
{
    if (!czk_relay_uniform)
        return;
    phase_cases(relay, {4224, 4144, 4136, 4129}, {4224, 4144, 4136, 4129}, 4129);
    phase_cases(relay, {144, 136, 133}, {256, 144, 133}, 133);
    for (uint32_t size : {0u, 1u, 32u, 33u, 255u, 256u, 257u, 4129u})
        for (uint64_t os : strides_for(size, false))
            relay(0, (size + 15u) & ~15ull, 0, os, 1000, size);
    for (uint32_t n : {1u, 63u, 64u, 65u, 127u, 128u, 129u, 1000u, 1024u, 1025u, 1u << 20})
        for (uint64_t os : {4224u, 4129u})
            relay(0, 4144, 0, os, n, 4129);
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        relay(0, 4144, 0, 4224, 1025, 4129);
        relay(1, 4129, 0, 4224, 1025, 4129);
        relay(0, 4144, 0, 4129, 1025, 4129);
    }
}

// The segmented relay's grid (`dispatch_record.py --relay-segments`; not part of the default record):
// segment counts around a workgroup, with and without split frames, every knob
void relay_segments_cases()
{
    if (!czk_relay_segments)
        return;
    for (const Knob &k : KNOBS) {
        WithKnob w(k);
        for (uint32_t nseg : {0u, 1u, 255u, 256u, 257u, 1025u, 1u << 20})
            for (uint32_t ncomb : {0u, 1u, 256u, 257u}) {
                const uint32_t npart = 2u * ncomb;
                std::printf("relay_segments nseg=%u ncomb=%u npart=%u\n", nseg, ncomb, npart);
                result(czk_relay_segments(ptr<cz_frame_desc>(AUX), ptr<cz_fanout_sub>(AUX + 2048), ptr<cz_segment>(AUX + 4096),
                                          nseg, ptr<cz_combine>(AUX + 8192), ncomb, npart, ptr<void>(IN), ptr<void>(OUT),
                                          ptr<void>(KEY), ptr<void>(AUX + 12288), ptr<uint16_t>(AUX + 16384),
                                          ptr<uint64_t>(AUX + 20480), nullptr));
            }
    }
}

// czk_tune: the old value it returns, what a value is clamped to, an unknown key
void tune_cases()
{
    for (const char *key : {"pair", "un0", "seglines", "shift", "open_ina", "seal_ina", "open_carry", "shift16", "nope"})
        for (int v : {-3, 0, 1, 2, 5}) {
            const int old = czk_tune(key, v), now = czk_tune(key, old < 0 ? 0 : old);
            std::printf("tune %s=%d old=%d set=%d\n", key, v, old, now);
        }
    std::printf("tune null old=%d\n", czk_tune(nullptr, 1));
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "relay") {
        relay_cases();
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "relay_segments") {
        relay_segments_cases();
        return 0;
    }
    seal_cases();
    open_cases();
    box_cases();
    fanout_cases();
    fanout_runs_cases();
    segment_cases();
    tune_cases();
    return 0;
}
