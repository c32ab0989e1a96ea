#!/usr/bin/env python3
"""PUB fan-out: one payload sealed for N subscribers, each under its own key and nonce.

Device legs (HIP-event time of back-to-back launches on device-resident buffers, one warm-up round,
median of --reps rounds, the legs interleaved inside every round), for N in {64, 1024, 16384, 2^18}
x len in {100, 4096}, plus len 65536 at N <= 16384; body slots of round_up(len + 33, 128) bytes,
one distinct key per subscriber:
  (a) cz_seal_fanout;
  (b) what the library offered before it: N descriptors sharing one in_off through
      cz_plan_segments + cz_seal_segments.  The host planning (descriptors + plan) and the metadata
      H2D are timed apart from the kernels (time.perf_counter around work that ends in a synchronise);
  (b') the same descriptors planned as cz_engine_flush_out would plan a flush that holds only this
      publish: segment length from the batch size (short segments for a small batch, so that a few
      frames spread over many lanes), kernels only;
  (c) cz_seal_uniform under ONE key at the same count and len (N payload slots): the yardstick a
      multi-key kernel cannot beat by much;
  (a') with --ab-lib: cz_seal_fanout of a second build of the library (tools/build_variant.sh),
      loaded into the same process and timed in the same rounds.

Engine leg: publish + flush_out of --engine-len bytes to --engine-conns connections x
--engine-msgs messages against the same traffic through per-connection send copies (the `engine`
config's shape: N x the arena bytes and H2D), wall clock, legs interleaved; the publish leg runs with
the fan-out routing forced on (cz_tune "fanout_min" = 64) and forced off (2^30); a pinned D2H copy of the
same wire bytes is timed beside them as the floor a flush cannot go below.

--runs measures the grouped fan-out instead (cz_plan_fanout + cz_seal_fanout_runs: all the publishes of a
flush group in one call), see runs_rows and engine_runs_leg: R runs x N subscribers x len on the device, and
the 256 x publish flush with the frames in the segment plan, routed by fanout_min 64, and routed by
fanout_short.

--split measures the split fan-out (cz_plan_fanout_split + cz_seal_fanout_split: lanes are (run, subscriber,
segment)), see split_rows and engine_split_leg: R runs x N subscribers x len on the device against the grouped
call and the segment kernels, and the 256 x publish flush in the segment plan against fanout_split = len.

Writes one JSON (default profiles/fanout/fanout.json, with --runs profiles/fanout/fanout_runs.json, with
--split profiles/fanout/fanout_split.json) and prints it."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (64, 1024, 16384, 1 << 18)
LENS = (100, 4096, 65536)
LONG_MAX_N = 16384


def round_up(v, a):
    return (v + a - 1) // a * a


def engine_seg_blocks(total, longest):
    """the segment length cz_engine_flush_out picks (batch_seg_blocks, cz_internal.h)"""
    s1 = 2
    while (s1 + 1) * (s1 + 1) * 18 <= longest:
        s1 += 1
    return min(128, max((total + 65535) // 65536, s1))


def event_ms(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def device_rows(args, torch, dev, batch, _lib, ab):
    L = _lib.lib()
    rows = []
    for length in args.lens:
        for n in args.sizes:
            if length > 4096 and n > LONG_MAX_N:
                continue
            stride = round_up(length + 33, 128)
            in_stride = round_up(length, 16)
            payload = torch.empty(round_up(length, 16) + 256, dtype=torch.uint8, device=dev)
            batch.fill(payload, 1)
            uni_in = torch.empty(n * in_stride + 256, dtype=torch.uint8, device=dev)
            batch.fill(uni_in, 2)
            sub = torch.empty(n * 32, dtype=torch.uint8, device=dev)
            batch.fill(sub, 3)
            sub = sub.view(n, 32)
            out = torch.empty(n * stride, dtype=torch.uint8, device=dev)
            rng = np.random.default_rng(n + length)
            subs = np.zeros(n, dtype=batch.FANOUT_SUB_DTYPE)
            subs["counter"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
            subs["key_idx"] = np.arange(n)
            d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)

            # (b) host planning and metadata H2D, timed apart
            def plan():
                desc = np.zeros(n, dtype=batch.DESC_DTYPE)
                desc["out_off"] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
                desc["len"] = length
                desc["key_idx"] = subs["key_idx"]
                desc["counter"] = subs["counter"]
                desc["prev"] = -1
                return desc, batch.SegmentPlan(desc, seg_blocks=args.seg_blocks or batch.SEG_BLOCKS)

            nblk = (length + 33 + 63) // 64
            short = engine_seg_blocks(n * nblk, nblk)

            def upload(desc, pl):
                d = torch.from_numpy(desc.view(np.uint8)).to(dev)
                pl.to(dev)
                torch.cuda.synchronize()
                return d

            t_plan, t_h2d = [], []
            for rep in range(args.reps + 1):
                t0 = time.perf_counter()
                desc, pl = plan()
                t1 = time.perf_counter()
                d_desc = upload(desc, pl)
                t2 = time.perf_counter()
                if rep:
                    t_plan.append(t1 - t0)
                    t_h2d.append(t2 - t1)
            pl_short = batch.SegmentPlan(desc, seg_blocks=short).to(dev)

            legs = {
                "fanout": lambda: batch.seal_fanout(payload, length, 0, d_subs, sub, out, stride, n),
                "segments": lambda: batch.seal_segments(d_desc, pl, payload, out, sub),
                "segments_short": lambda: batch.seal_segments(d_desc, pl_short, payload, out, sub),
                "uniform": lambda: batch.seal_uniform(uni_in, in_stride, out, stride, n, length, sub[0], 7),
            }
            if ab is not None:
                stream = torch.cuda.current_stream().cuda_stream
                legs["fanout_ab"] = lambda: _lib.check(ab.cz_seal_fanout(
                    n, length, payload.data_ptr(), 0, d_subs.data_ptr(), sub.data_ptr(), out.data_ptr(), stride, stream))
            # sanity at the timed shape: the legs that seal the same frames agree
            legs["fanout"]()
            got = out.clone()
            legs["segments"]()
            torch.cuda.synchronize()
            assert torch.equal(got.view(n, stride)[:, :length + 33], out.view(n, stride)[:, :length + 33]), \
                "cz_seal_fanout and cz_seal_segments disagree"
            del got
            inner = {}
            for k, fn in legs.items():     # warm-up, and enough launches for a ~2 ms window
                inner[k] = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, fn, 1), 1e-3))))
            times = {k: [] for k in legs}
            for rep in range(args.reps):
                for k, fn in legs.items():
                    times[k].append(event_ms(torch, fn, inner[k]))
            body_bytes = n * (length + 33)
            row = {"n": n, "len": length, "out_stride": stride, "segments": pl.nseg, "combines": pl.ncomb,
                   "short_seg_blocks": short, "short_segments": pl_short.nseg,
                   "plan_host_ms": round(statistics.median(t_plan) * 1e3, 4),
                   "plan_h2d_ms": round(statistics.median(t_h2d) * 1e3, 4),
                   "plan_metadata_bytes": int(desc.nbytes + pl.segments.nbytes + pl.combines.nbytes),
                   "fanout_metadata_bytes": int(subs.nbytes)}
            for k in legs:
                med = statistics.median(times[k])
                row[k + "_ms"] = round(med, 5)
                row[k + "_all_ms"] = [round(t, 5) for t in times[k]]
                row[k + "_gib_s"] = round(body_bytes / (med * 1e-3) / 2**30, 2)
                row[k + "_launches_per_window"] = inner[k]
            rows.append(row)
            print(f"n={n} len={length}: " + ", ".join(f"{k} {row[k + '_ms']} ms" for k in legs), file=sys.stderr)
            del payload, uni_in, sub, out, d_subs, d_desc, pl, pl_short
            torch.cuda.empty_cache()
    return rows


RUNS_R = (1, 16, 256)
RUNS_N = (64, 1024)
RUNS_LENS = (100, 256, 1024, 4096)


def runs_rows(args, torch, dev, batch, _lib):
    """--runs, device legs: R runs x N subscribers x len (R payloads, the same N keys for every run, counters
    per (run, subscriber), slots of round_up(len + 33, 128)), same method as device_rows:
      (d)   one cz_seal_fanout_runs call (at most three launches);
      (axR) R cz_seal_fanout launches back to back (ctypes calls with prepared arguments);
      (b')  the same R x N descriptors through cz_seal_segments at the segment length a flush of that size picks."""
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for length in args.runs_lens:
        for n in args.runs_n:
            for nr in args.runs_r:
                stride = round_up(length + 33, 128)
                pstride = round_up(length, 16) + 16
                payload = torch.empty(nr * pstride + 256, dtype=torch.uint8, device=dev)
                batch.fill(payload, 1)
                sub = torch.empty(n * 32, dtype=torch.uint8, device=dev)
                batch.fill(sub, 3)
                sub = sub.view(n, 32)
                out = torch.empty(nr * n * stride, dtype=torch.uint8, device=dev)
                rng = np.random.default_rng(nr * n + length)
                subs = np.zeros(nr * n, dtype=batch.FANOUT_SUB_DTYPE)
                subs["counter"] = rng.integers(0, 1 << 63, size=nr * n, dtype=np.uint64)
                subs["key_idx"] = np.tile(np.arange(n), nr)
                d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
                runs = np.zeros(nr, dtype=batch.FANOUT_RUN_DTYPE)
                runs["payload_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(pstride)
                runs["out_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(n * stride)
                runs["out_stride"], runs["len"], runs["count"] = stride, length, n
                runs["first_sub"] = np.arange(nr) * n
                t0 = time.perf_counter()
                plan = batch.plan_fanout(runs, payload, out)
                t_plan = time.perf_counter() - t0
                plan.to(dev)
                desc = np.zeros(nr * n, dtype=batch.DESC_DTYPE)
                desc["in_off"] = np.repeat(runs["payload_off"], n)
                desc["out_off"] = np.arange(nr * n, dtype=np.uint64) * np.uint64(stride)
                desc["len"], desc["prev"] = length, -1
                desc["key_idx"], desc["counter"] = subs["key_idx"], subs["counter"]
                nblk = (length + 33 + 63) // 64
                short = engine_seg_blocks(nr * n * nblk, nblk)
                pl_short = batch.SegmentPlan(desc, seg_blocks=short).to(dev)
                d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
                calls = [(n, length, payload.data_ptr() + r * pstride, 0, d_subs.data_ptr() + 16 * r * n, sub.data_ptr(),
                          out.data_ptr() + r * n * stride, stride, stream) for r in range(nr)]
                seal_one = L.cz_seal_fanout

                def back_to_back():
                    for a in calls:
                        if seal_one(*a):
                            raise RuntimeError(_lib.last_error())

                # (prepared ctypes calls for (d) too: the Python wrapper's bounds checks cost more host time than
                # the launch takes on the device, and the events would time the host)
                seal_runs = L.cz_seal_fanout_runs
                grouped_args = (plan.d_runs.data_ptr(), nr, plan.d_waves.data_ptr(),
                                (ctypes.c_uint32 * 3)(*plan.class_count), plan.region_stride, payload.data_ptr(),
                                d_subs.data_ptr(), sub.data_ptr(), out.data_ptr(), stream)

                def grouped():
                    if seal_runs(*grouped_args):
                        raise RuntimeError(_lib.last_error())

                batch.seal_fanout_runs(plan, payload, d_subs, sub, out)   # (the checked wrapper once: bounds)
                legs = {"grouped": grouped,
                        "fanout_x_r": back_to_back,
                        "segments_short": lambda: batch.seal_segments(d_desc, pl_short, payload, out, sub)}
                # sanity at the timed shape: the three legs write the same bodies
                legs["segments_short"]()
                want = out.clone()
                for k in ("grouped", "fanout_x_r"):
                    out.zero_()
                    legs[k]()
                    torch.cuda.synchronize()
                    assert torch.equal(want.view(nr * n, stride)[:, :length + 33], out.view(nr * n, stride)[:, :length + 33]), \
                        f"{k} and cz_seal_segments disagree"
                del want
                inner = {}
                for k, fn in legs.items():     # warm-up, and enough calls for a ~2 ms window
                    inner[k] = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, fn, 1), 1e-3))))
                times = {k: [] for k in legs}
                for rep in range(args.reps):
                    for k, fn in legs.items():
                        times[k].append(event_ms(torch, fn, inner[k]))
                row = {"runs": nr, "n": n, "lanes": nr * n, "len": length, "out_stride": stride, "waves": plan.nwaves,
                       "class_count": plan.class_count, "plan_host_ms": round(t_plan * 1e3, 4),
                       "grouped_metadata_bytes": int(runs.nbytes + plan.waves.nbytes + subs.nbytes),
                       "short_seg_blocks": short, "short_segments": pl_short.nseg}
                for k in legs:
                    med = statistics.median(times[k])
                    row[k + "_ms"] = round(med, 5)
                    row[k + "_all_ms"] = [round(t, 5) for t in times[k]]
                    row[k + "_calls_per_window"] = inner[k]
                rows.append(row)
                print(f"R={nr} n={n} len={length}: " + ", ".join(f"{k} {row[k + '_ms']} ms" for k in legs), file=sys.stderr)
                del payload, sub, out, d_subs, d_desc, pl_short, plan
                torch.cuda.empty_cache()
    return rows


def engine_runs_leg(args, _lib, length):
    """--runs, engine leg: --engine-msgs x publish of `length` bytes to --engine-conns connections, flushed with
    the frames left in the segment plan, with fanout_min 64, and with fanout_short = length (fanout_min at its
    default); wall clock of flush_out, one warm-up round, legs interleaved."""
    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    nc, nm = args.engine_conns, args.engine_msgs
    body = length + 33
    wire_bytes = nc * nm * (body + (9 if body > 255 else 2))
    payloads = [np.random.default_rng(m).integers(0, 256, size=length, dtype=np.uint8).tobytes() for m in range(nm)]
    eng = CurveBatchEngine(arena_bytes=nm * round_up(length, 16) + 4096)
    cc = [eng.add_connection(np.random.default_rng(1000 + i).integers(0, 256, size=32, dtype=np.uint8).tobytes())
          for i in range(nc)]
    ids = (ctypes.c_int * nc)(*cc)
    default_min = L.cz_tune(b"fanout_min", 1 << 30)
    L.cz_tune(b"fanout_min", default_min)
    routings = {"segments": (1 << 30, 0), "fanout_min_64": (64, 0), "fanout_short": (default_min, length)}

    def run(fmin, fshort):
        old = L.cz_tune(b"fanout_min", fmin), L.cz_tune(b"fanout_short", fshort)
        try:
            for p in payloads:
                _lib.check(L.cz_engine_publish(eng._h, ids, nc, p, length, 0, None), "cz_engine_publish")
            t0 = time.perf_counter()
            eng.flush_out()
            return time.perf_counter() - t0
        finally:
            L.cz_tune(b"fanout_min", old[0])
            L.cz_tune(b"fanout_short", old[1])

    res = {k: [] for k in routings}
    for rep in range(args.reps + 1):
        for k, (fmin, fshort) in routings.items():
            t = run(fmin, fshort)
            if rep:
                res[k].append(t)
    eng.close()
    out = {"connections": nc, "messages": nm, "len": length, "wire_bytes": wire_bytes, "clock": "time.perf_counter"}
    for k, v in res.items():
        out[k + "_flush_ms"] = round(statistics.median(v) * 1e3, 3)
        out[k + "_flush_all_ms"] = [round(t * 1e3, 3) for t in v]
    return out


def fanout_short_rule(rows, engines):
    """The rule that sets the shipped fanout_short: the largest measured length at which the grouped call is not
    slower than (b') in the median at every measured R x N >= 1024 and the engine flush routed by fanout_short is
    not slower than the segment-plan flush of the same run -- and every shorter measured length qualifies too
    (the knob routes everything up to its value); 0 if none."""
    verdict = {}
    for length in sorted({r["len"] for r in rows}):
        dev_ok = all(r["grouped_ms"] <= r["segments_short_ms"] for r in rows if r["len"] == length and r["lanes"] >= 1024)
        eng = [e for e in engines if e["len"] == length]
        eng_ok = bool(eng) and all(e["fanout_short_flush_ms"] <= e["segments_flush_ms"] for e in eng)
        verdict[str(length)] = {"device": dev_ok, "engine": eng_ok if eng else None}
    best = 0
    for length in sorted(int(k) for k in verdict):
        if not (verdict[str(length)]["device"] and verdict[str(length)]["engine"]):
            break
        best = length
    return verdict, best


SPLIT_SHAPES = ((1, 64), (16, 64), (1, 1024), (16, 1024), (256, 1024))   # R x N
SPLIT_LENS = (1024, 4096, 16384, 65536)


def split_rows(args, torch, dev, batch, _lib):
    """--split, device legs: R runs x N subscribers x len, laid out as runs_rows lays them out, same method:
      (e)   one cz_seal_fanout_split call at the segment length a flush of that size picks (at most three launches);
      (d)   one cz_seal_fanout_runs call;
      (b')  the same R x N descriptors through cz_seal_segments at the same segment length, its host planning
            (descriptors + cz_plan_segments) timed beside it, and the metadata bytes of (e) and (b')."""
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for length in args.split_lens:
        for nr, n in SPLIT_SHAPES:
            stride = round_up(length + 33, 128)
            pstride = round_up(length, 16) + 16
            payload = torch.empty(nr * pstride + 256, dtype=torch.uint8, device=dev)
            batch.fill(payload, 1)
            sub = torch.empty(n * 32, dtype=torch.uint8, device=dev)
            batch.fill(sub, 3)
            sub = sub.view(n, 32)
            out = torch.empty(nr * n * stride, dtype=torch.uint8, device=dev)
            rng = np.random.default_rng(nr * n + length)
            subs = np.zeros(nr * n, dtype=batch.FANOUT_SUB_DTYPE)
            subs["counter"] = rng.integers(0, 1 << 63, size=nr * n, dtype=np.uint64)
            subs["key_idx"] = np.tile(np.arange(n), nr)
            d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
            runs = np.zeros(nr, dtype=batch.FANOUT_RUN_DTYPE)
            runs["payload_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(pstride)
            runs["out_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(n * stride)
            runs["out_stride"], runs["len"], runs["count"] = stride, length, n
            runs["first_sub"] = np.arange(nr) * n
            nblk = (length + 33 + 63) // 64
            seg = engine_seg_blocks(nr * n * nblk, nblk)
            t0 = time.perf_counter()
            sp = batch.plan_fanout_split(runs, payload, out, seg)
            t_split_plan = time.perf_counter() - t0
            sp.to(dev)
            work = torch.empty(64 * max(sp.npart, 1), dtype=torch.uint8, device=dev)
            gp = batch.plan_fanout(runs, payload, out).to(dev)

            def plan_segments():
                desc = np.zeros(nr * n, dtype=batch.DESC_DTYPE)
                desc["in_off"] = np.repeat(runs["payload_off"], n)
                desc["out_off"] = np.arange(nr * n, dtype=np.uint64) * np.uint64(stride)
                desc["len"], desc["prev"] = length, -1
                desc["key_idx"], desc["counter"] = subs["key_idx"], subs["counter"]
                return desc, batch.SegmentPlan(desc, seg_blocks=seg)

            t_plan = []
            for rep in range(3):
                t0 = time.perf_counter()
                desc, pl = plan_segments()
                t_plan.append(time.perf_counter() - t0)
            pl.to(dev)
            d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
            # prepared ctypes calls: the wrappers' bounds checks cost more host time than a small launch takes
            seal_split, seal_runs, seal_segs = L.cz_seal_fanout_split, L.cz_seal_fanout_runs, L.cz_seal_segments
            split_args = (sp.d_runs.data_ptr(), nr, sp.d_tiles.data_ptr(), (ctypes.c_uint32 * 2)(*sp.class_count),
                          sp.d_joins.data_ptr(), len(sp.joins), payload.data_ptr(), d_subs.data_ptr(), sub.data_ptr(),
                          out.data_ptr(), work.data_ptr(), stream)
            grouped_args = (gp.d_runs.data_ptr(), nr, gp.d_waves.data_ptr(), (ctypes.c_uint32 * 3)(*gp.class_count),
                            gp.region_stride, payload.data_ptr(), d_subs.data_ptr(), sub.data_ptr(), out.data_ptr(), stream)
            seg_args = (d_desc.data_ptr(), pl.d_seg.data_ptr(), pl.nseg, pl.d_comb.data_ptr(), pl.ncomb,
                        payload.data_ptr(), out.data_ptr(), sub.data_ptr(), pl.d_work.data_ptr(), stream)

            def call(f, a):
                def go():
                    if f(*a):
                        raise RuntimeError(_lib.last_error())
                return go

            batch.seal_fanout_split(sp, payload, d_subs, sub, out, work=work)   # (the checked wrapper once: bounds)
            legs = {"split": call(seal_split, split_args), "grouped": call(seal_runs, grouped_args),
                    "segments_short": call(seal_segs, seg_args)}
            # sanity at the timed shape: the three legs write the same bodies
            legs["segments_short"]()
            want = out.clone()
            for k in ("split", "grouped"):
                out.zero_()
                legs[k]()
                torch.cuda.synchronize()
                assert torch.equal(want.view(nr * n, stride)[:, :length + 33], out.view(nr * n, stride)[:, :length + 33]), \
                    f"{k} and cz_seal_segments disagree"
            del want
            inner = {}
            for k, fn in legs.items():     # warm-up, and enough calls for a ~2 ms window
                inner[k] = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, fn, 1), 1e-3))))
            times = {k: [] for k in legs}
            for rep in range(args.reps):
                for k, fn in legs.items():
                    times[k].append(event_ms(torch, fn, inner[k]))
            row = {"runs": nr, "n": n, "lanes": nr * n, "len": length, "out_stride": stride, "seg_blocks": seg,
                   "tiles": len(sp.tiles), "tile_class_count": sp.class_count, "joins": len(sp.joins), "npart": sp.npart,
                   "split_plan_host_ms": round(t_split_plan * 1e3, 4),
                   "split_metadata_bytes": int(runs.nbytes + sp.tiles.nbytes + sp.joins.nbytes + subs.nbytes),
                   "segments": pl.nseg, "combines": pl.ncomb,
                   "segments_plan_host_ms": round(statistics.median(t_plan) * 1e3, 4),
                   "segments_metadata_bytes": int(desc.nbytes + pl.segments.nbytes + pl.combines.nbytes)}
            for k in legs:
                med = statistics.median(times[k])
                row[k + "_ms"] = round(med, 5)
                row[k + "_all_ms"] = [round(t, 5) for t in times[k]]
                row[k + "_calls_per_window"] = inner[k]
            rows.append(row)
            print(f"R={nr} n={n} len={length} seg={seg}: " + ", ".join(f"{k} {row[k + '_ms']} ms" for k in legs),
                  file=sys.stderr)
            del payload, sub, out, d_subs, d_desc, pl, sp, gp, work
            torch.cuda.empty_cache()
    return rows


def engine_split_leg(args, _lib, length):
    """--split, engine leg: --engine-msgs x publish of `length` bytes to --engine-conns connections, flushed with
    the frames in the segment plan (fanout_split 0) and with fanout_split = length; wall clock of flush_out, one
    warm-up round, legs interleaved."""
    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    nc, nm = args.engine_conns, args.engine_msgs
    body = length + 33
    wire_bytes = nc * nm * (body + (9 if body > 255 else 2))
    payloads = [np.random.default_rng(m).integers(0, 256, size=length, dtype=np.uint8).tobytes() for m in range(nm)]
    eng = CurveBatchEngine(arena_bytes=nm * round_up(length, 16) + 4096)
    cc = [eng.add_connection(np.random.default_rng(1000 + i).integers(0, 256, size=32, dtype=np.uint8).tobytes())
          for i in range(nc)]
    ids = (ctypes.c_int * nc)(*cc)
    routings = {"segments": 0, "fanout_split": length}

    def run(split):
        old = L.cz_tune(b"fanout_split", split)
        try:
            for p in payloads:
                _lib.check(L.cz_engine_publish(eng._h, ids, nc, p, length, 0, None), "cz_engine_publish")
            t0 = time.perf_counter()
            eng.flush_out()
            return time.perf_counter() - t0
        finally:
            L.cz_tune(b"fanout_split", old)

    res = {k: [] for k in routings}
    for rep in range(args.reps + 1):
        for k, split in routings.items():
            t = run(split)
            if rep:
                res[k].append(t)
    eng.close()
    out = {"connections": nc, "messages": nm, "len": length, "wire_bytes": wire_bytes, "clock": "time.perf_counter"}
    for k, v in res.items():
        out[k + "_flush_ms"] = round(statistics.median(v) * 1e3, 3)
        out[k + "_flush_all_ms"] = [round(t * 1e3, 3) for t in v]
    print(f"engine len={length}: " + ", ".join(f"{k} {out[k + '_flush_ms']} ms" for k in routings), file=sys.stderr)
    return out


def fanout_split_rule(rows, engines):
    """The rule that sets the shipped fanout_split, fixed before the run: the smallest measured length L such that,
    for every measured length >= L, the split call is not slower than (b') in the median at every measured
    R x N >= 1024 lanes and the flush routed by fanout_split is not slower than the segment-plan flush; 0 if no
    length qualifies."""
    verdict = {}
    for length in sorted({r["len"] for r in rows}):
        dev_ok = all(r["split_ms"] <= r["segments_short_ms"] for r in rows if r["len"] == length and r["lanes"] >= 1024)
        eng = [e for e in engines if e["len"] == length]
        eng_ok = bool(eng) and all(e["fanout_split_flush_ms"] <= e["segments_flush_ms"] for e in eng)
        verdict[str(length)] = {"device": dev_ok, "engine": eng_ok if eng else None}
    best = 0
    for length in sorted((int(k) for k in verdict), reverse=True):
        if not (verdict[str(length)]["device"] and verdict[str(length)]["engine"]):
            break
        best = length
    return verdict, best


def engine_leg(args, torch, _lib):
    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    nc, nm, length = args.engine_conns, args.engine_msgs, args.engine_len
    body = length + 33
    wire_bytes = nc * nm * (body + (9 if body > 255 else 2))
    payloads = [np.random.default_rng(m).integers(0, 256, size=length, dtype=np.uint8).tobytes() for m in range(nm)]

    def make(arena):
        e = CurveBatchEngine(arena_bytes=arena)
        cc = [e.add_connection(np.random.default_rng(1000 + i).integers(0, 256, size=32, dtype=np.uint8).tobytes())
              for i in range(nc)]
        return e, cc

    pub, pc = make(nm * round_up(length, 16) + 4096)
    snd, sc = make(nc * nm * round_up(length, 16) + 4096)
    ids = (ctypes.c_int * nc)(*pc)

    def run_publish(fanout_min):
        old = L.cz_tune(b"fanout_min", fanout_min)
        try:
            t0 = time.perf_counter()
            for p in payloads:
                _lib.check(L.cz_engine_publish(pub._h, ids, nc, p, length, 0, None), "cz_engine_publish")
            t1 = time.perf_counter()
            pub.flush_out()
            return t1 - t0, time.perf_counter() - t1
        finally:
            L.cz_tune(b"fanout_min", old)

    def run_send():
        t0 = time.perf_counter()
        send, h = L.cz_engine_send, snd._h
        for p in payloads:
            for c in sc:
                if send(h, c, p, length, 0):
                    raise RuntimeError("cz_engine_send failed: " + _lib.last_error())
        t1 = time.perf_counter()
        snd.flush_out()
        return t1 - t0, time.perf_counter() - t1

    d_wire = torch.empty(wire_bytes, dtype=torch.uint8, device="cuda:0")
    h_wire = torch.empty(wire_bytes, dtype=torch.uint8).pin_memory()

    def run_d2h():
        t0 = time.perf_counter()
        h_wire.copy_(d_wire, non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    res = {"publish_queue": [], "publish_fanout_flush": [], "publish_segments_flush": [], "send_queue": [],
           "send_flush": [], "d2h": []}
    for rep in range(args.reps + 1):
        pq, pf = run_publish(64)
        _, ps = run_publish(1 << 30)
        sq, sf = run_send()
        d = run_d2h()
        if rep == 0:
            continue
        for k, v in zip(res, (pq, pf, ps, sq, sf, d)):
            res[k].append(v)
    out = {"connections": nc, "messages": nm, "len": length, "wire_bytes": wire_bytes,
           "fanout_min_default": L.cz_tune(b"fanout_min", 64), "clock": "time.perf_counter",
           "publish_arena_bytes": nm * round_up(length, 16), "send_arena_bytes": nc * nm * round_up(length, 16)}
    L.cz_tune(b"fanout_min", out["fanout_min_default"])
    for k, v in res.items():
        out[k + "_ms"] = round(statistics.median(v) * 1e3, 3)
        out[k + "_all_ms"] = [round(t * 1e3, 3) for t in v]
    for k in ("publish_fanout_flush", "publish_segments_flush", "send_flush", "d2h"):
        out[k + "_gib_s"] = round(wire_bytes / statistics.median(res[k]) / 2**30, 2)
    pub.close()
    snd.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--lens", type=int, nargs="*", default=list(LENS))
    ap.add_argument("--seg-blocks", type=int, default=0, help="segment length of leg (b) (default: the library's)")
    ap.add_argument("--ab-lib", default=None, help="a second build of the library: its cz_seal_fanout as leg (a')")
    ap.add_argument("--ab-name", default=None, help="what the second build is (recorded in the JSON)")
    ap.add_argument("--engine-conns", type=int, default=1024)
    ap.add_argument("--engine-msgs", type=int, default=256)
    ap.add_argument("--engine-len", type=int, default=4096)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-device", action="store_true", help="skip the device legs")
    ap.add_argument("--runs", action="store_true",
                    help="the grouped fan-out instead: R runs x N subscribers (default --out: fanout_runs.json)")
    ap.add_argument("--runs-r", type=int, nargs="*", default=list(RUNS_R))
    ap.add_argument("--runs-n", type=int, nargs="*", default=list(RUNS_N))
    ap.add_argument("--runs-lens", type=int, nargs="*", default=list(RUNS_LENS))
    ap.add_argument("--engine-runs-lens", type=int, nargs="*", default=list(RUNS_LENS))
    ap.add_argument("--split", action="store_true",
                    help="the split fan-out instead: subscriber x segment grid (default --out: fanout_split.json)")
    ap.add_argument("--split-lens", type=int, nargs="*", default=list(SPLIT_LENS))
    ap.add_argument("--engine-split-lens", type=int, nargs="*", default=list(SPLIT_LENS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "fanout", "fanout_split.json" if args.split else
                                        "fanout_runs.json" if args.runs else "fanout.json")
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from jeromq_amd import _lib, batch, build
    assert torch.cuda.is_available(), "fanout_bench needs a GPU"
    dev = torch.device("cuda:0")
    ab = None
    if args.ab_lib:
        ab = ctypes.CDLL(os.path.abspath(args.ab_lib))
        ab.cz_seal_fanout.restype, ab.cz_seal_fanout.argtypes = _lib.SIGNATURES["cz_seal_fanout"]
    kernels = ["k_seal_fanout<1, true>", "k_seal_fanout<2, false>", "k_seal_fanout<0, true>"]
    out = {"device": torch.cuda.get_device_name(0), "library": _lib.lib().cz_version().decode(),
           "fanout_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, kernels), "reps": args.reps,
           "clock_device": "hipEvent (torch.cuda.Event), median", "ab_lib": args.ab_name or args.ab_lib}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if args.split:
        out["fanout_runs_kernels_sha256"] = build.kernel_code_sha256(
            _lib.LIB_PATH, [k.replace("k_seal_fanout<", "k_seal_fanout_runs<") for k in kernels])
        out["fanout_split_kernels_sha256"] = build.kernel_code_sha256(
            _lib.LIB_PATH, ["k_seal_fanout_tiles<1>", "k_seal_fanout_tiles<0>", "k_fanout_join"])
        out["segment_kernels_sha256"] = build.kernel_code_sha256(
            _lib.LIB_PATH, ["k_seal_segments_lines", "k_seal_segments", "k_seal_combine"])
        out["fanout_split_default"] = _lib.lib().cz_tune(b"fanout_split", 0)
        _lib.lib().cz_tune(b"fanout_split", out["fanout_split_default"])
        if not args.no_device:
            out["split_legs"] = split_rows(args, torch, dev, batch, _lib)
            write()   # (kept if an engine leg below cannot get its buffers)
        if not args.no_engine:
            out["engine_split"] = []
            for length in args.engine_split_lens:
                out["engine_split"].append(engine_split_leg(args, _lib, length))
                write()
        if "split_legs" in out and "engine_split" in out:
            out["fanout_split_verdict"], out["fanout_split_rule"] = fanout_split_rule(out["split_legs"], out["engine_split"])
    elif args.runs:
        out["fanout_runs_kernels_sha256"] = build.kernel_code_sha256(
            _lib.LIB_PATH, [k.replace("k_seal_fanout<", "k_seal_fanout_runs<") for k in kernels])
        out["fanout_short_default"] = _lib.lib().cz_tune(b"fanout_short", 0)
        _lib.lib().cz_tune(b"fanout_short", out["fanout_short_default"])
        if not args.no_device:
            out["runs_legs"] = runs_rows(args, torch, dev, batch, _lib)
        if not args.no_engine:
            out["engine_runs"] = [engine_runs_leg(args, _lib, length) for length in args.engine_runs_lens]
        if "runs_legs" in out and "engine_runs" in out:
            out["fanout_short_verdict"], out["fanout_short_rule"] = fanout_short_rule(out["runs_legs"], out["engine_runs"])
    elif not args.no_device:
        out["device_legs"] = device_rows(args, torch, dev, batch, _lib, ab)
    if not args.no_engine and not args.runs and not args.split:
        out["engine"] = engine_leg(args, torch, _lib)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
