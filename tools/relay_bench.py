#!/usr/bin/env python3
"""CURVE relay (cz_relay_uniform / cz_relay_batch, header section 3h) against the two calls it replaces.

Every leg interleaves the relay with the two-call path in one process: shapes warmed, --reps (at least 10)
alternations, the median and the spread of each side reported, and the outputs of both sides compared at the
timed size (byte-equal bodies, every frame accepted).  The yardstick is the two-call path on the same build.

Device legs (HIP events around one call of each side):
  uniform  cz_relay_uniform  against  cz_open_uniform into 4224- / 144-byte plaintext slots, then cz_seal_uniform
           2^20 x 4129-byte bodies in 4224-byte slots; 2^20 x 133-byte bodies in 144-byte slots;
           2^20 x 4129-byte bodies at the dense stride 4129
  batch    cz_relay_batch    against  cz_open_batch then cz_seal_batch, the same descriptors
           2^16 frames of 1 KiB payload under 1024 key pairs
Host-staged leg (pinned torch tensors, one stream, a host clock ending in a synchronise), 2^16 x 4 KiB:
  relay     H2D bodies -> cz_relay_uniform -> D2H bodies
  two-call  H2D bodies -> open -> D2H payloads -> H2D payloads -> seal -> D2H bodies

--segments measures the segmented relay (cz_relay_segments, header section 3i) instead and writes
profiles/relay/relay_segments.json; the legs above and relay.json are not touched.  Three sides alternate, all
at seg_blocks = batch.SEG_BLOCKS:
  A  cz_relay_segments on the cz_plan_segments(open = 1) plan
  B  cz_relay_batch with cz_plan_order (one lane per frame, longest first)
  C  cz_open_segments, then cz_seal_segments
over 1024 bodies of 65569 bytes under 1024 key pairs; 2^16 frames of the Zipf 64 B .. 64 KiB length mix of
bench.py's zipf config; 2^16 bodies of 1 KiB payload (nothing is split).  16-byte aligned slots.

--streams measures the stream relay (cz_relay_streams, header section 3j) and the engine's forward routes instead
and writes profiles/relay/relay_streams.json.  Device leg, 1024 streams x 16 frames of 100 B, 1 KiB and 4 KiB
payloads and 64 streams x 1 frame of 4 KiB, four sides alternating: cz_relay_streams in place and out of place,
cz_open_streams + cz_seal_batch + cz_v2_copy(CZ_V2_ITEM_HEADER), and the host parse + cz_relay_batch.  Engine leg,
1024 routes x 16 frames: cz_engine_flush_forward against flush_in + send of every message + flush_out on a second
broker fed the same bytes.

Writes profiles/relay/relay.json and prints it.  --log2 / --batch-log2 / --host-log2 shrink the shapes for a
rehearsal; the committed file is measured at the defaults.  --pmc: one call of each side at the first uniform
shape, for a counter run:
  rocprofv3 --pmc SQ_INSTS_VALU --output-format csv -d DIR -o run -- python3 tools/relay_bench.py --pmc"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ["k_relay_uniform<1>", "k_relay_uniform<0>", "k_relay_desc"]
# (name, body size, in_stride, out_stride, plaintext stride)
UNIFORM_SHAPES = (("4k_slots", 4129, 4224, 4224, 4224), ("100b_slots", 133, 144, 144, 144),
                  ("4k_dense", 4129, 4129, 4129, 4224))


def round_up(v, a):
    return (v + a - 1) // a * a


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(torch, clock, legs, reps):
    """warm every leg once, then `reps` alternations; per leg the median, the extremes and the spread"""
    for fn in legs.values():
        clock(torch, fn)
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(clock(torch, fn))
    row = {}
    for k, t in times.items():
        med = statistics.median(t)
        row[k + "_ms"] = round(med, 5)
        row[k + "_min_ms"], row[k + "_max_ms"] = round(min(t), 5), round(max(t), 5)
        row[k + "_spread"] = round((max(t) - min(t)) / med, 4)
        row[k + "_all_ms"] = [round(v, 5) for v in t]
    return row


def finish(row, body_bytes):
    row["relay_over_two_call"] = round(row["relay_ms"] / row["two_call_ms"], 4)
    row["relay_gib_s"] = round(body_bytes / 2**30 / (row["relay_ms"] * 1e-3), 1)
    row["two_call_gib_s"] = round(body_bytes / 2**30 / (row["two_call_ms"] * 1e-3), 1)
    return row


def make_bodies(torch, batch, dev, count, size, stride, key, counter0, scratch_stride):
    """`count` MESSAGE bodies of `size` bytes at `stride`, sealed on the device from synthetic payloads"""
    length = size - 33
    plain = torch.empty(count * scratch_stride + 64, dtype=torch.uint8, device=dev)
    batch.fill(plain, 11)
    bodies = torch.zeros(count * stride + 64, dtype=torch.uint8, device=dev)
    batch.seal_uniform(plain, scratch_stride, bodies, stride, count, length, key, counter0)
    return bodies, plain


def uniform_leg(args, torch, dev, batch, name, size, ist, ost, pst, once=False):
    count = 1 << args.log2
    keys = torch.empty(64, dtype=torch.uint8, device=dev)
    batch.fill(keys, 5)
    k_in, k_out = keys[:32], keys[32:]
    floor0, counter0 = (1 << 33) + 5, (7 << 32) - 1000
    bodies, plain = make_bodies(torch, batch, dev, count, size, ist, k_in, floor0 + 1, pst)
    out_r = torch.zeros(count * ost + 64, dtype=torch.uint8, device=dev)
    out_t = torch.zeros(count * ost + 64, dtype=torch.uint8, device=dev)
    st_r = torch.full((count,), -1, dtype=torch.int16, device=dev)
    st_t = torch.full((count,), -1, dtype=torch.int16, device=dev)
    n_in, n_out = (count - 1) * ist + size, count * ost if ost % 16 == 0 else (count - 1) * ost + size

    def relay():
        batch.relay_uniform(bodies[:n_in], ist, out_r[:n_out], ost, count, size, k_in, floor0, k_out, counter0, st_r)

    def two_call():
        batch.open_uniform(bodies[:n_in], ist, plain, pst, count, size, k_in, floor0, st_t)
        batch.seal_uniform(plain, pst, out_t[:n_out], ost, count, size - 33, k_out, counter0)

    relay()
    two_call()
    torch.cuda.synchronize()
    assert int((st_r != 0).sum()) == 0 and int((st_t != 0).sum()) == 0, "a body was rejected"
    assert torch.equal(out_r, out_t), "cz_relay_uniform and open + seal disagree"
    if once:
        return None
    row = {"leg": name, "count": count, "size": size, "in_stride": ist, "out_stride": ost, "plain_stride": pst}
    row.update(alternate(torch, event_ms, {"relay": relay, "two_call": two_call}, args.reps))
    return finish(row, count * size)


def batch_leg(args, torch, dev, batch):
    count, pairs, length = 1 << args.batch_log2, 1024, 1024
    size, slot, pslot = length + 33, round_up(length + 33, 16), round_up(length, 16)
    keys = torch.empty(2 * pairs * 32, dtype=torch.uint8, device=dev)
    batch.fill(keys, 7)
    keys = keys.view(2 * pairs, 32)
    idx = np.arange(count, dtype=np.uint64)
    k_in = (2 * (idx % pairs)).astype(np.uint32)
    k_out = (2 * ((idx * 7 + 1) % pairs) + 1).astype(np.uint32)
    plain = torch.empty(count * pslot + 64, dtype=torch.uint8, device=dev)
    batch.fill(plain, 13)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    # the received bodies: sealed under the inbound keys
    sd = np.zeros(count, dtype=batch.DESC_DTYPE)
    sd["in_off"], sd["out_off"], sd["len"], sd["key_idx"] = idx * pslot, idx * slot, length, k_in
    sd["counter"], sd["prev"] = idx + 100, -1
    bodies = torch.zeros(count * slot + 64, dtype=torch.uint8, device=dev)
    batch.seal_batch(up(sd), count, plain, bodies, keys, desc_np=sd)
    # relay / open descriptors (the same records), the outbound records, and the second call's seal descriptors
    od = np.zeros(count, dtype=batch.DESC_DTYPE)
    od["in_off"], od["len"], od["key_idx"], od["counter"] = idx * slot, size, k_in, idx + 99
    od["flags"], od["prev"] = 0x100, -1
    rd = od.copy()
    rd["out_off"] = idx * slot
    od["out_off"] = idx * pslot
    to = np.zeros(count, dtype=batch.FANOUT_SUB_DTYPE)
    to["counter"], to["key_idx"] = idx + (1 << 40), k_out
    td = sd.copy()
    td["key_idx"], td["counter"] = k_out, to["counter"]
    d_rd, d_od, d_to, d_td = up(rd), up(od), up(to), up(td)
    out_r = torch.zeros(count * slot + 64, dtype=torch.uint8, device=dev)
    out_t = torch.zeros(count * slot + 64, dtype=torch.uint8, device=dev)
    st_r = torch.full((count,), -1, dtype=torch.int16, device=dev)
    st_t = torch.full((count,), -1, dtype=torch.int16, device=dev)

    def relay():
        batch.relay_batch(d_rd, d_to, count, bodies, out_r, keys, st_r)

    def two_call():
        batch.open_batch(d_od, count, bodies, plain, keys, st_t)
        batch.seal_batch(d_td, count, plain, out_t, keys)

    batch.relay_batch(d_rd, d_to, count, bodies, out_r, keys, st_r, desc_np=rd, to_np=to)      # bounds, once
    two_call()
    torch.cuda.synchronize()
    assert int((st_r != 0).sum()) == 0 and int((st_t != 0).sum()) == 0, "a body was rejected"
    assert torch.equal(out_r, out_t), "cz_relay_batch and open_batch + seal_batch disagree"
    row = {"leg": "batch_1k_1024_pairs", "count": count, "size": size, "key_pairs": pairs, "slot": slot}
    row.update(alternate(torch, event_ms, {"relay": relay, "two_call": two_call}, args.reps))
    return finish(row, count * size)


SEGMENT_KERNELS = ["k_relay_segments", "k_relay_combine", "k_relay_desc"]


def zipf_lengths(frames):
    """bench.py's zipf config: payload lengths 64 j, j ~ Zipf(1.2) on 1..1024, seed 42"""
    rng = np.random.default_rng(42)
    j = np.empty(0, dtype=np.int64)
    while len(j) < frames:
        z = rng.zipf(1.2, size=frames)
        j = np.concatenate([j, z[z <= 1024]])
    return (64 * j[:frames]).astype(np.uint64)


def segments_leg(args, torch, dev, batch, name, lengths):
    """payload lengths -> bodies sealed under 1024 inbound keys in 16-byte aligned slots, then the three sides"""
    count, pairs = len(lengths), 1024
    lengths = np.asarray(lengths, dtype=np.uint64)
    sizes = lengths + np.uint64(33)
    off = lambda ln: np.concatenate([[0], np.cumsum((ln + np.uint64(15)) // np.uint64(16) * np.uint64(16))]).astype(np.uint64)  # noqa: E731
    poff, boff = off(lengths), off(sizes)
    keys = torch.empty(2 * pairs * 32, dtype=torch.uint8, device=dev)
    batch.fill(keys, 7)
    keys = keys.view(2 * pairs, 32)
    idx = np.arange(count, dtype=np.uint64)
    k_in = (2 * (idx % pairs)).astype(np.uint32)
    k_out = (2 * ((idx * 7 + 1) % pairs) + 1).astype(np.uint32)
    plain = torch.empty(int(poff[-1]) + 64, dtype=torch.uint8, device=dev)
    batch.fill(plain, 13)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    sb = batch.SEG_BLOCKS
    # the received bodies: sealed under the inbound keys
    sd = np.zeros(count, dtype=batch.DESC_DTYPE)
    sd["in_off"], sd["out_off"], sd["len"], sd["key_idx"] = poff[:-1], boff[:-1], lengths, k_in
    sd["counter"], sd["prev"] = idx + 100, -1
    bodies = torch.zeros(int(boff[-1]) + 64, dtype=torch.uint8, device=dev)
    batch.seal_segments(up(sd), batch.SegmentPlan(sd, open_=False, seg_blocks=sb).to(dev), plain, bodies, keys, desc_np=sd)
    # relay / open descriptors (the same records), the outbound records, and side C's seal descriptors
    od = np.zeros(count, dtype=batch.DESC_DTYPE)
    od["in_off"], od["len"], od["key_idx"], od["counter"] = boff[:-1], sizes, k_in, idx + 99
    od["flags"], od["prev"] = 0x100, -1
    rd = od.copy()
    rd["out_off"] = boff[:-1]
    od["out_off"] = poff[:-1]
    to = np.zeros(count, dtype=batch.FANOUT_SUB_DTYPE)
    to["counter"], to["key_idx"] = idx + (1 << 40), k_out
    td = sd.copy()
    td["key_idx"], td["counter"] = k_out, to["counter"]
    d_rd, d_od, d_to, d_td = up(rd), up(od), up(to), up(td)
    plan_a = batch.SegmentPlan(rd, open_=True, seg_blocks=sb).to(dev, records=2)
    plan_o = batch.SegmentPlan(od, open_=True, seg_blocks=sb).to(dev)
    plan_s = batch.SegmentPlan(td, open_=False, seg_blocks=sb).to(dev)
    d_order = torch.from_numpy(batch.plan_order(rd).view(np.int32)).to(dev)
    outs = [torch.zeros(int(boff[-1]) + 64, dtype=torch.uint8, device=dev) for _ in range(3)]
    sts = [torch.full((count,), -1, dtype=torch.int16, device=dev) for _ in range(3)]

    def side_a():
        batch.relay_segments(d_rd, d_to, plan_a, bodies, outs[0], keys, sts[0])

    def side_b():
        batch.relay_batch(d_rd, d_to, count, bodies, outs[1], keys, sts[1], order=d_order)

    def side_c():
        batch.open_segments(d_od, plan_o, bodies, plain, keys, sts[2])
        batch.seal_segments(d_td, plan_s, plain, outs[2], keys)

    batch.relay_segments(d_rd, d_to, plan_a, bodies, outs[0], keys, sts[0], desc_np=rd, to_np=to)      # bounds, once
    side_b()
    side_c()
    torch.cuda.synchronize()
    assert all(int((st != 0).sum()) == 0 for st in sts), "a body was rejected"
    assert torch.equal(outs[0], outs[1]), "cz_relay_segments and cz_relay_batch disagree"
    assert torch.equal(outs[0], outs[2]), "cz_relay_segments and open_segments + seal_segments disagree"
    body_bytes = int(sizes.sum())
    row = {"leg": name, "count": count, "body_bytes": body_bytes, "max_size": int(sizes.max()), "key_pairs": pairs,
           "seg_blocks": sb, "segments": plan_a.nseg, "split_frames": plan_a.ncomb}
    row.update(alternate(torch, event_ms, {"segments": side_a, "batch": side_b, "open_seal": side_c}, args.reps))
    row["a_over_b"] = round(row["segments_ms"] / row["batch_ms"], 4)
    row["a_over_c"] = round(row["segments_ms"] / row["open_seal_ms"], 4)
    for k in ("segments", "batch", "open_seal"):
        row[k + "_gib_s"] = round(body_bytes / 2**30 / (row[k + "_ms"] * 1e-3), 1)
    return row


def segments_main(args, torch, dev, batch, build, _lib):
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().cz_version().decode(),
           "relay_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, SEGMENT_KERNELS), "reps": args.reps,
           "sides": {"segments": "A: cz_relay_segments", "batch": "B: cz_relay_batch with cz_plan_order",
                     "open_seal": "C: cz_open_segments then cz_seal_segments"},
           "clock_device": "hipEvent (torch.cuda.Event) around one call of each side, median of the alternations",
           "spread": "(max - min) / median of a side's alternations", "legs": []}
    path = args.out if args.out else os.path.join(ROOT, "profiles", "relay", "relay_segments.json")
    n = 1 << args.seg_log2
    shapes = (("64k_x_1024", np.full(min(1024, n), 65536, dtype=np.uint64)), ("zipf", zipf_lengths(n)),
              ("1k_unsplit", np.full(n, 1024, dtype=np.uint64)))
    for name, lengths in shapes:
        out["legs"].append(segments_leg(args, torch, dev, batch, name, lengths))
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for r in out["legs"]:
        print(f"{r['leg']}: A {r['segments_ms']} ms, B {r['batch_ms']} ms, C {r['open_seal_ms']} ms, A/B {r['a_over_b']}, "
              f"A/C {r['a_over_c']}", file=sys.stderr)
    print(json.dumps({k: v for k, v in out.items() if k != "legs"} |
                     {"legs": [{k: v for k, v in r.items() if not k.endswith("_all_ms")} for r in out["legs"]]}))


STREAM_KERNELS = ["k_v2_scan", "k_v2_place", "k_v2_emit_relay", "k_relay_desc", "k_relay_cut"]
# (name, streams, frames per stream, payload bytes)
STREAM_SHAPES = (("1024x16_100b", 1024, 16, 100), ("1024x16_1k", 1024, 16, 1024), ("1024x16_4k", 1024, 16, 4096),
                 ("64x1_4k", 64, 1, 4096))


def prepared(torch, legs, reps):
    """alternate() for legs that need their input restored first: legs = {name: (prepare, fn)}; only fn is timed
    (a host clock between two synchronisations: every side synchronises inside or is short)"""
    def once(prep, fn):
        prep()
        return wall_ms(torch, fn)
    for prep, fn in legs.values():
        once(prep, fn)
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, (prep, fn) in legs.items():
            times[k].append(once(prep, fn))
    row = {}
    for k, t in times.items():
        med = statistics.median(t)
        row[k + "_ms"] = round(med, 5)
        row[k + "_min_ms"], row[k + "_max_ms"] = round(min(t), 5), round(max(t), 5)
        row[k + "_spread"] = round((max(t) - min(t)) / med, 4)
        row[k + "_all_ms"] = [round(v, 5) for v in t]
    return row


def streams_device_leg(args, torch, dev, batch, wire, name, nstreams, nframes, length):
    """`nstreams` received streams of `nframes` frames, each under its own key pair, packed back to back.
    in_place / out_of_place: cz_relay_streams.  open_seal_pack: cz_open_streams, cz_seal_batch, cz_v2_copy with
    CZ_V2_ITEM_HEADER, the seal's descriptors and the copy's items built once outside the clock.  host_parse:
    cz_v2_parse per stream on the host, descriptors with prev chains built and uploaded, cz_relay_batch."""
    size = length + 33
    hdr = 9 if size > 255 else 2
    count = nstreams * nframes
    keys = torch.empty(2 * nstreams * 32, dtype=torch.uint8, device=dev)
    batch.fill(keys, 7)
    keys = keys.view(2 * nstreams, 32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)  # noqa: E731
    idx = np.arange(count, dtype=np.uint64)
    s_of, k_of = idx // np.uint64(nframes), idx % np.uint64(nframes)
    pslot, bslot, fb = round_up(max(length, 1), 128), round_up(size, 16), hdr + size
    # the received wire: payloads sealed under the inbound keys, packed behind their V2 headers
    plain = torch.empty(count * pslot + 64, dtype=torch.uint8, device=dev)
    batch.fill(plain, 13)
    sd = np.zeros(count, dtype=batch.DESC_DTYPE)
    sd["in_off"], sd["out_off"], sd["len"], sd["key_idx"] = idx * pslot, idx * bslot, length, 2 * s_of
    sd["counter"], sd["prev"] = 100 + k_of, -1
    bodies = torch.zeros(count * bslot + 64, dtype=torch.uint8, device=dev)
    batch.seal_batch(up(sd), count, plain, bodies, keys, desc_np=sd)
    items = np.zeros(count, dtype=wire.V2_ITEM_DTYPE)
    items["src_off"], items["dst_off"], items["size"], items["flags"] = idx * bslot, idx * fb, size, 0x100
    d_items = up(items)
    total = count * fb
    orig = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    wire.copy(d_items, bodies, orig)
    st = np.zeros(nstreams, dtype=wire.V2_STREAM_DTYPE)
    st["off"], st["len"] = np.arange(nstreams, dtype=np.uint64) * (nframes * fb), nframes * fb
    st["floor"], st["key_idx"] = 99, 2 * np.arange(nstreams)
    to = np.zeros(nstreams, dtype=batch.FANOUT_SUB_DTYPE)
    to["counter"], to["key_idx"] = 1 << 40, 2 * ((np.arange(nstreams) * 7 + 1) % nstreams) + 1
    d_st, d_to = wire.to_device(st, dev), wire.to_device(to, dev)
    z = lambda n: torch.zeros(n, dtype=torch.uint8, device=dev)  # noqa: E731
    work, outs = orig.clone(), {k: z(total + 64) for k in ("out_of_place", "open_seal_pack", "host_parse")}
    scan, cut, desc, tof = z(nstreams * 32), z(nstreams * 32), z(count * 40), z(count * 16)
    status = {k: torch.full((count,), -1, dtype=torch.int16, device=dev)
              for k in ("in_place", "out_of_place", "open_seal_pack", "host_parse")}
    nonces = torch.zeros(count, dtype=torch.int64, device=dev)
    # side B's second and third call: seal from the open's plaintext slots into body slots, pack behind headers
    td = sd.copy()
    td["key_idx"], td["counter"] = to["key_idx"][s_of.astype(np.int64)], (1 << 40) + k_of
    d_td, body2 = up(td), z(count * bslot + 64)
    h_wire = orig.cpu().numpy()
    nothing = lambda: None  # noqa: E731

    def in_place():
        batch.relay_streams(d_st, d_to, work, work, scan, desc, tof, keys, status["in_place"], nonces, cut)

    def out_of_place():
        batch.relay_streams(d_st, d_to, orig, outs["out_of_place"], scan, desc, tof, keys, status["out_of_place"], nonces,
                            cut)

    def open_seal_pack():
        batch.open_streams(d_st, orig, scan, desc, plain, keys, status["open_seal_pack"], nonces=nonces, slot_align=128)
        batch.seal_batch(d_td, count, plain, body2, keys)
        wire.copy(d_items, body2, outs["open_seal_pack"])

    def host_parse():
        rd = np.zeros(count, dtype=batch.DESC_DTYPE)
        at = 0
        for s in range(nstreams):
            o, n = int(st["off"][s]), int(st["len"][s])
            frames, _consumed, _rc = wire.parse(h_wire[o:o + n], cap=nframes + 1)
            r = rd[at:at + len(frames)]
            r["in_off"] = r["out_off"] = frames["body_off"] + np.uint64(o)
            r["len"], r["key_idx"], r["counter"], r["flags"] = frames["size"], st["key_idx"][s], 99, 0x100
            r["prev"] = np.arange(at - 1, at - 1 + len(frames))
            r["prev"][0] = -1
            at += len(frames)
        tf = np.zeros(count, dtype=batch.FANOUT_SUB_DTYPE)
        tf["counter"], tf["key_idx"] = td["counter"], td["key_idx"]
        batch.relay_batch(up(rd), up(tf), count, orig, outs["host_parse"], keys, status["host_parse"])

    legs = {"in_place": (lambda: work.copy_(orig), in_place), "out_of_place": (nothing, out_of_place),
            "open_seal_pack": (nothing, open_seal_pack), "host_parse": (nothing, host_parse)}
    for prep, fn in legs.values():
        prep()
        fn()
    torch.cuda.synchronize()
    assert all(int((s != 0).sum()) == 0 for s in status.values()), "a body was rejected"
    assert torch.equal(work[:total], outs["out_of_place"][:total]), "in place and out of place disagree"
    assert torch.equal(work[:total], outs["open_seal_pack"][:total]), "cz_relay_streams and open + seal + pack disagree"
    b = outs["host_parse"].view(-1)[:total].view(count, fb)[:, hdr:]
    assert torch.equal(work[:total].view(count, fb)[:, hdr:], b), "cz_relay_streams and parse + cz_relay_batch disagree"
    row = {"leg": name, "streams": nstreams, "frames_per_stream": nframes, "payload": length, "wire_bytes": total}
    row.update(prepared(torch, legs, args.reps))
    for k in ("in_place", "out_of_place"):
        row[k + "_over_open_seal_pack"] = round(row[k + "_ms"] / row["open_seal_pack_ms"], 4)
        row[k + "_over_host_parse"] = round(row[k + "_ms"] / row["host_parse_ms"], 4)
    return row


def streams_engine_leg(args, torch, _lib, name, nroutes, nframes, length):
    """flush_forward of `nroutes` routes x `nframes` frames against flush_in + cz_engine_send of every delivered
    message + flush_out on a second broker; a peer engine makes fresh traffic for every repetition, and both
    brokers have received it before the clock starts.  two_flushes: the second broker's two flush calls alone."""
    import ctypes

    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    arena = max(1 << 22, 2 * nroutes * nframes * (length + 64))
    peer, br, br2 = (CurveBatchEngine(arena_bytes=arena) for _ in range(3))
    pre = bytes(range(32))
    p = peer.add_connections([pre] * nroutes, as_server=False)
    ends = []
    for e in (br, br2):
        src = e.add_connections([pre] * nroutes, as_server=True)
        dst = e.add_connections([pre] * nroutes, as_server=True)
        ends.append((src, dst))
    for s, d in zip(*ends[0]):
        br.forward(s, d)
    payload = bytes(length)
    t = {"forward": [], "flush_in_send_flush_out": [], "two_flushes": []}
    pp, n, fl = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_int()
    cnt = ctypes.c_uint32()
    for rep in range(args.reps + 1):
        for c in p:
            for _ in range(nframes):
                peer.send(c, payload)
        peer.flush_out()
        for k, c in enumerate(p):
            w = peer.wire_out(c)
            br.recv(ends[0][0][k], w)
            br2.recv(ends[1][0][k], w)
        f_ms = wall_ms(torch, br.flush_forward)
        t0 = time.perf_counter()
        br2.flush_in()
        t1 = time.perf_counter()
        for s, d in zip(*ends[1]):
            L.cz_engine_msgs_in(br2._h, s, ctypes.byref(cnt))
            for i in range(cnt.value):
                L.cz_engine_msg_in(br2._h, s, i, ctypes.byref(pp), ctypes.byref(n), ctypes.byref(fl))
                L.cz_engine_send(br2._h, d, pp, n, fl)
        t2 = time.perf_counter()
        br2.flush_out()
        t3 = time.perf_counter()
        assert br.forward_frames == nroutes * nframes
        same = all(br.forward_out(s) == br2.wire_out(d) for s, d in list(zip(ends[0][0], ends[1][1]))[:8])
        assert same, "flush_forward and flush_in + send + flush_out disagree"
        if rep:     # (the first round warms both)
            t["forward"].append(f_ms)
            t["flush_in_send_flush_out"].append((t3 - t0) * 1e3)
            t["two_flushes"].append((t1 - t0 + t3 - t2) * 1e3)
    for e in (peer, br, br2):
        e.close()
    row = {"leg": name, "routes": nroutes, "frames_per_route": nframes, "payload": length}
    for k, v in t.items():
        med = statistics.median(v)
        row[k + "_ms"], row[k + "_spread"] = round(med, 4), round((max(v) - min(v)) / med, 4)
        row[k + "_all_ms"] = [round(x, 4) for x in v]
    row["forward_over_flush_in_send_flush_out"] = round(row["forward_ms"] / row["flush_in_send_flush_out_ms"], 4)
    row["forward_over_two_flushes"] = round(row["forward_ms"] / row["two_flushes_ms"], 4)
    return row


def streams_main(args, torch, dev, batch, build, _lib):
    from jeromq_amd import wire
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().cz_version().decode(),
           "stream_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, STREAM_KERNELS), "reps": args.reps,
           "sides": {"in_place": "cz_relay_streams, d_out = d_wire (the wire restored outside the clock)",
                     "out_of_place": "cz_relay_streams into a second buffer",
                     "open_seal_pack": "cz_open_streams, cz_seal_batch, cz_v2_copy with CZ_V2_ITEM_HEADER; the seal's "
                                       "descriptors and the copy's items are built outside the clock",
                     "host_parse": "cz_v2_parse per stream (driven from Python), descriptors with prev chains built and "
                                   "uploaded, cz_relay_batch",
                     "forward": "cz_engine_flush_forward",
                     "flush_in_send_flush_out": "cz_engine_flush_in, cz_engine_msg_in + cz_engine_send of every message "
                                                "through ctypes, cz_engine_flush_out on a second broker",
                     "two_flushes": "that broker's flush_in and flush_out alone, the send loop left out"},
           "clock": "time.perf_counter between two synchronisations around one call of a side, median of the alternations",
           "spread": "(max - min) / median of a side's alternations", "legs": [], "engine_legs": []}
    path = args.out if args.out else os.path.join(ROOT, "profiles", "relay", "relay_streams.json")

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    shrink = args.streams_shrink
    for name, ns, nf, length in STREAM_SHAPES:
        out["legs"].append(streams_device_leg(args, torch, dev, batch, wire, name, max(ns // shrink, 1), nf, length))
        torch.cuda.empty_cache()
        write()
    for name, ns, nf, length in STREAM_SHAPES[:3]:
        out["engine_legs"].append(streams_engine_leg(args, torch, _lib, name, max(ns // shrink, 1), nf, length))
        write()
    for r in out["legs"]:
        print(f"{r['leg']}: in place {r['in_place_ms']} ms, out of place {r['out_of_place_ms']} ms, open + seal + pack "
              f"{r['open_seal_pack_ms']} ms, host parse + relay {r['host_parse_ms']} ms", file=sys.stderr)
    for r in out["engine_legs"]:
        print(f"engine {r['leg']}: forward {r['forward_ms']} ms, flush_in + send + flush_out "
              f"{r['flush_in_send_flush_out_ms']} ms, the two flushes alone {r['two_flushes_ms']} ms", file=sys.stderr)
    strip = lambda rows: [{k: v for k, v in r.items() if not k.endswith("_all_ms")} for r in rows]  # noqa: E731
    print(json.dumps({k: v for k, v in out.items() if k not in ("legs", "engine_legs")} |
                     {"legs": strip(out["legs"]), "engine_legs": strip(out["engine_legs"])}))


def host_leg(args, torch, dev, batch):
    count, size, ist, pst = 1 << args.host_log2, 4129, 4224, 4096
    keys = torch.empty(64, dtype=torch.uint8, device=dev)
    batch.fill(keys, 9)
    k_in, k_out = keys[:32], keys[32:]
    floor0, counter0 = 77, 1 << 35
    d_bodies, _ = make_bodies(torch, batch, dev, count, size, ist, k_in, floor0 + 1, ist)
    nb, npl = count * ist, count * pst
    h_in = torch.empty(nb, dtype=torch.uint8).pin_memory()
    h_in.copy_(d_bodies[:nb])
    h_out_r, h_out_t = torch.zeros(nb, dtype=torch.uint8).pin_memory(), torch.zeros(nb, dtype=torch.uint8).pin_memory()
    h_plain = torch.zeros(npl, dtype=torch.uint8).pin_memory()
    d_in = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_plain = torch.zeros(npl, dtype=torch.uint8, device=dev)
    st_r = torch.full((count,), -1, dtype=torch.int16, device=dev)
    st_t = torch.full((count,), -1, dtype=torch.int16, device=dev)

    def relay():
        d_in.copy_(h_in, non_blocking=True)
        batch.relay_uniform(d_in, ist, d_out, ist, count, size, k_in, floor0, k_out, counter0, st_r)
        h_out_r.copy_(d_out, non_blocking=True)

    def two_call():
        d_in.copy_(h_in, non_blocking=True)
        batch.open_uniform(d_in, ist, d_plain, pst, count, size, k_in, floor0, st_t)
        h_plain.copy_(d_plain, non_blocking=True)
        d_plain.copy_(h_plain, non_blocking=True)
        batch.seal_uniform(d_plain, pst, d_out, ist, count, size - 33, k_out, counter0)
        h_out_t.copy_(d_out, non_blocking=True)

    relay()
    two_call()
    torch.cuda.synchronize()
    assert int((st_r != 0).sum()) == 0 and int((st_t != 0).sum()) == 0, "a body was rejected"
    assert torch.equal(h_out_r, h_out_t), "the host-staged relay and open + seal disagree"
    row = {"leg": "host_staged_4k", "count": count, "size": size, "stride": ist, "plain_stride": pst,
           "relay_pcie_bytes": 2 * nb, "two_call_pcie_bytes": 2 * nb + 2 * npl}
    row.update(alternate(torch, wall_ms, {"relay": relay, "two_call": two_call}, args.reps))
    return finish(row, count * size)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=12, help="alternations per leg (at least 10; --segments: at least 12)")
    ap.add_argument("--log2", type=int, default=20, help="uniform legs: log2 of the frame count")
    ap.add_argument("--batch-log2", type=int, default=16)
    ap.add_argument("--host-log2", type=int, default=16)
    ap.add_argument("--pmc", action="store_true",
                    help="one call of each side at the first uniform shape and nothing else: the run to put under "
                         "rocprofv3 --pmc SQ_INSTS_VALU (counters in a run of their own, no tracing)")
    ap.add_argument("--segments", action="store_true",
                    help="measure cz_relay_segments against cz_relay_batch and open_segments + seal_segments instead; "
                         "writes profiles/relay/relay_segments.json")
    ap.add_argument("--seg-log2", type=int, default=16, help="--segments: log2 of the frame count of the ragged legs")
    ap.add_argument("--streams", action="store_true",
                    help="measure cz_relay_streams and cz_engine_flush_forward against the routes they replace instead; "
                         "writes profiles/relay/relay_streams.json")
    ap.add_argument("--streams-shrink", type=int, default=1, help="--streams: divide the stream counts (a rehearsal)")
    ap.add_argument("--out", default=None, help="default: profiles/relay/relay.json (relay_segments.json with --segments, "
                                                "relay_streams.json with --streams)")
    args = ap.parse_args()
    if args.reps < (12 if args.segments else 10):
        ap.error("--reps: at least 10 alternations (--segments: 12)")
    import torch

    from jeromq_amd import _lib, batch, build
    if not torch.cuda.is_available():
        raise SystemExit("relay_bench needs a GPU")
    dev = torch.device("cuda:0")
    if args.segments:
        segments_main(args, torch, dev, batch, build, _lib)
        return
    if args.streams:
        streams_main(args, torch, dev, batch, build, _lib)
        return
    args.out = args.out or os.path.join(ROOT, "profiles", "relay", "relay.json")
    if args.pmc:
        uniform_leg(args, torch, dev, batch, *UNIFORM_SHAPES[0], once=True)
        return
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().cz_version().decode(),
           "relay_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, KERNELS), "reps": args.reps,
           "clock_device": "hipEvent (torch.cuda.Event) around one call of each side, median of the alternations",
           "clock_host": "time.perf_counter around the copies and calls, ending in a synchronise, median",
           "spread": "(max - min) / median of a side's alternations", "legs": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for shape in UNIFORM_SHAPES:
        out["legs"].append(uniform_leg(args, torch, dev, batch, *shape))
        torch.cuda.empty_cache()
        write()
    out["legs"].append(batch_leg(args, torch, dev, batch))
    write()
    out["legs"].append(host_leg(args, torch, dev, batch))
    write()
    for r in out["legs"]:
        print(f"{r['leg']}: relay {r['relay_ms']} ms, two calls {r['two_call_ms']} ms, ratio {r['relay_over_two_call']}",
              file=sys.stderr)
    print(json.dumps({k: v for k, v in out.items() if k != "legs"} |
                     {"legs": [{k: v for k, v in r.items() if not k.endswith("_all_ms")} for r in out["legs"]]}))


if __name__ == "__main__":
    main()
