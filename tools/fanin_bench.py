#!/usr/bin/env python3
"""Fan-in open (cz_open_fanin_runs, header section 3f) against the paths received frames take without it.

Device legs, R runs x N bodies x len (R in --runs-r, N in --runs-n, len = payload bytes in --lens): the bodies are
real MESSAGE bodies (sealed on the device: run r is one payload for N connections, each under its own key, so
connection j's chain is body j of run 0, 1, ...), in 128-byte multiple slots as cz_engine_flush_in lays them out;
HIP events around enough back-to-back calls for a ~2 ms window, median of --reps windows after a warm-up, legs
interleaved:
  (a) one cz_open_fanin_runs call (at most three launches): run 0 above plain floors, every later body above the
      wire nonce of its connection's previous body (FLOOR_IS_BODY);
  (b) cz_open_segments on the same bodies: descriptors with the same chains as `prev`, at the segment length
      cz_engine_flush_in picks for that many bytes -- the path the frames take today;
  (c) cz_open_uniform of R x N bodies of the same payloads sealed under ONE key (a second set of slots, so that
      every tag verifies), as the ceiling.
Engine legs, --engine-conns connections x --engine-frames received frames of each length: wall clock of flush_in
with fanin_short = len against fanin_short = 0 on two engines fed the same wire, one warm-up round, legs
interleaved.  With --ab-lib (a build of the parent commit, tools/build_variant.sh) the same flush is timed once more
in a child process that loads that library (CZ_LIB), to confirm that the off leg is the parent's code path.

The rule that sets the shipped fanin_short (the one that set fanout_short): the largest measured length at which (a)
is not slower than (b) in the median at every measured R x N >= 1024 and the routed flush is not slower than the
unrouted one -- every shorter measured length qualifying too; 0 if none.

Writes profiles/fanin/fanin.json and prints it.  These legs run with fanin_split at 0, so that they keep measuring
the fan-in call against the segment plan alone.

--split: the split fan-in (cz_open_fanin_split, header section 3g) instead, into profiles/fanin/fanin_split.json.
Device legs at payload lengths 1024, 4096, 16 384 and 65 536 and R x N = 1 x 64, 16 x 64, 1 x 1024, 16 x 1024 and
256 x 1024, the same bodies, clocks and interleaving as above:
  (e) one cz_open_fanin_split call (at most three launches) at the segment length a flush of that size picks;
  (a) one cz_open_fanin_runs call;
  (b) cz_open_segments on the same bodies with the same chains as `prev`, at the same segment length;
with the host plan time and the metadata bytes of (e) against (b).  Engine legs: flush_in of --engine-conns
connections x 16 and x 256 frames with fanin_split = len against fanin_split = 0 on two engines fed the same wire.
The rule that sets the shipped fanin_split (the one that set fanout_split): the smallest measured length L such that
at every measured length >= L (e) is not slower than (b) in the median at every measured R x N >= 1024 and the
routed flush is not slower than the unrouted one at both engine shapes; 0 (the rule is off) if none."""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS_R = (1, 16, 256)
RUNS_N = (64, 1024, 16384)
LENS = (100, 256, 1024, 4096)
SPLIT_LENS = (1024, 4096, 16384, 65536)
SPLIT_SHAPES = ((1, 64), (16, 64), (1, 1024), (16, 1024), (256, 1024))   # R x N
SPLIT_ENGINE_FRAMES = (16, 256)
SPLIT_KERNELS = ["k_open_fanin_tiles<1>", "k_open_fanin_tiles<0>", "k_fanin_join"]
KERNELS = ["k_open_fanin_runs<1, true>", "k_open_fanin_runs<2, false>", "k_open_fanin_runs<0, true>"]


def round_up(v, a):
    return (v + a - 1) // a * a


def flush_seg_blocks(wire_bytes):
    """the segment length cz_engine_flush_in picks (flush_seg_blocks, cz_engine.cpp)"""
    return min(128, max(4, (wire_bytes // 64 + 65535) // 65536))


def event_ms(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def device_rows(args, torch, dev, batch, _lib):
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for length in args.lens:
        size = length + 33
        bstride, pstride = round_up(size, 128), round_up(max(length, 1), 128)
        for n in args.runs_n:
            for nr in args.runs_r:
                if nr * n * (2 * bstride + 2 * pstride) > args.max_bytes:
                    continue
                total = nr * n
                keys = torch.empty(n * 32, dtype=torch.uint8, device=dev)
                batch.fill(keys, 3)
                keys = keys.view(n, 32)
                payload = torch.empty(nr * round_up(length, 16) + 256, dtype=torch.uint8, device=dev)
                batch.fill(payload, 1)
                bodies = torch.zeros(total * bstride, dtype=torch.uint8, device=dev)
                out = torch.empty(total * pstride, dtype=torch.uint8, device=dev)
                rng = np.random.default_rng(total + length)
                base = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
                # the bodies: run r = one payload sealed for the n connections, counter base + r + 1
                ssubs = np.zeros(total, dtype=batch.FANOUT_SUB_DTYPE)
                ssubs["counter"] = (np.tile(base, nr) + np.repeat(np.arange(1, nr + 1, dtype=np.uint64), n))
                ssubs["key_idx"] = np.tile(np.arange(n), nr)
                sruns = np.zeros(nr, dtype=batch.FANOUT_RUN_DTYPE)
                sruns["payload_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(round_up(length, 16))
                sruns["out_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(n * bstride)
                sruns["out_stride"], sruns["len"], sruns["count"] = bstride, length, n
                sruns["first_sub"] = np.arange(nr) * n
                splan = batch.plan_fanout(sruns, payload, bodies).to(dev)
                batch.seal_fanout_runs(splan, payload, torch.from_numpy(ssubs.view(np.uint8).copy()).to(dev), keys, bodies)
                # ... and the same bodies under key 0 alone, for leg (c)
                bodies_c = torch.zeros(total * bstride, dtype=torch.uint8, device=dev)
                csubs = ssubs.copy()
                csubs["key_idx"] = 0
                batch.seal_fanout_runs(splan, payload, torch.from_numpy(csubs.view(np.uint8).copy()).to(dev), keys, bodies_c)
                del splan
                # (a) records and runs
                subs = np.zeros(total, dtype=batch.FANIN_SUB_DTYPE)
                subs["key_idx"] = ssubs["key_idx"]
                subs["flags"] = batch.FANIN_CHECK_NONCE | batch.FANIN_FLOOR_IS_BODY
                subs["floor"] = (np.arange(total, dtype=np.uint64) - np.uint64(n)) * np.uint64(bstride)
                subs["floor"][:n], subs["flags"][:n] = base, batch.FANIN_CHECK_NONCE
                d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
                runs = np.zeros(nr, dtype=batch.FANIN_RUN_DTYPE)
                runs["in_off"], runs["out_off"] = sruns["out_off"], np.arange(nr, dtype=np.uint64) * np.uint64(n * pstride)
                runs["in_stride"], runs["out_stride"], runs["size"], runs["count"] = bstride, pstride, size, n
                runs["first_sub"] = np.arange(nr) * n
                t0 = time.perf_counter()
                plan = batch.plan_fanin(runs, bodies, out)
                t_plan = time.perf_counter() - t0
                plan.to(dev)
                status = torch.zeros(total, dtype=torch.int16, device=dev)
                nonces = torch.zeros(total, dtype=torch.int64, device=dev)
                # (b) descriptors with the same chains, the engine's segment length
                desc = np.zeros(total, dtype=batch.DESC_DTYPE)
                desc["in_off"] = np.arange(total, dtype=np.uint64) * np.uint64(bstride)
                desc["out_off"] = np.arange(total, dtype=np.uint64) * np.uint64(pstride)
                desc["len"], desc["key_idx"], desc["flags"] = size, ssubs["key_idx"], 0x100
                desc["counter"] = np.tile(base, nr)
                desc["prev"] = np.arange(total, dtype=np.int64) - n
                desc["prev"][:n] = -1
                wire = total * (size + (9 if size > 255 else 2))
                seg = args.seg_blocks or flush_seg_blocks(wire)
                pl = batch.SegmentPlan(desc, open_=True, seg_blocks=seg).to(dev)
                d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
                st_b = torch.zeros(total, dtype=torch.int16, device=dev)
                nn_b = torch.zeros(total, dtype=torch.int64, device=dev)
                st_c = torch.zeros(total, dtype=torch.int16, device=dev)
                open_runs = L.cz_open_fanin_runs
                a_args = (plan.d_runs.data_ptr(), nr, plan.d_waves.data_ptr(), (ctypes.c_uint32 * 3)(*plan.class_count),
                          plan.region_stride, bodies.data_ptr(), d_subs.data_ptr(), keys.data_ptr(), out.data_ptr(),
                          status.data_ptr(), nonces.data_ptr(), stream)

                def fanin():
                    if open_runs(*a_args):
                        raise RuntimeError(_lib.last_error())

                batch.open_fanin_runs(plan, bodies, d_subs, keys, out, status, nonces=nonces, subs_np=subs)  # bounds, once
                legs = {"fanin": fanin,
                        "segments": lambda: batch.open_segments(d_desc, pl, bodies, out, keys, st_b, nonces=nn_b),
                        "uniform_one_key": lambda: batch.open_uniform(bodies_c, bstride, out, pstride, total, size, keys[0],
                                                                      0, st_c, check=False)}
                # sanity at the timed shape: (a) and (b) accept every body and write the same plaintext
                legs["segments"]()
                want = out.clone()
                out.zero_()
                fanin()
                torch.cuda.synchronize()
                assert int((status != st_b).sum()) == 0 and int((status.view(torch.uint8)[::2] != 0).sum()) == 0, \
                    "statuses differ or a body was rejected"
                assert torch.equal(nonces, nn_b), "nonces differ"
                assert torch.equal(want.view(total, pstride)[:, :length], out.view(total, pstride)[:, :length]), \
                    "cz_open_fanin_runs and cz_open_segments disagree"
                legs["uniform_one_key"]()
                torch.cuda.synchronize()
                assert int((st_c != status).sum()) == 0, "the one-key bodies were not all accepted"
                assert torch.equal(want.view(total, pstride)[:, :length], out.view(total, pstride)[:, :length])
                del want
                inner = {}
                for k, fn in legs.items():     # warm-up, and enough calls for a ~2 ms window
                    inner[k] = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, fn, 1), 1e-3))))
                times = {k: [] for k in legs}
                for rep in range(args.reps):
                    for k, fn in legs.items():
                        times[k].append(event_ms(torch, fn, inner[k]))
                row = {"runs": nr, "n": n, "lanes": total, "len": length, "size": size, "in_stride": bstride,
                       "out_stride": pstride, "waves": plan.nwaves, "class_count": plan.class_count,
                       "plan_host_ms": round(t_plan * 1e3, 4),
                       "fanin_metadata_bytes": int(runs.nbytes + plan.waves.nbytes + subs.nbytes),
                       "segments_metadata_bytes": int(desc.nbytes + pl.nseg * 16 + pl.ncomb * 16),
                       "seg_blocks": seg, "segments": pl.nseg}
                for k in legs:
                    row[k + "_ms"] = round(statistics.median(times[k]), 5)
                    row[k + "_all_ms"] = [round(t, 5) for t in times[k]]
                    row[k + "_calls_per_window"] = inner[k]
                rows.append(row)
                print(f"R={nr} n={n} len={length}: " + ", ".join(f"{k} {row[k + '_ms']} ms" for k in legs), file=sys.stderr)
                del keys, payload, bodies, bodies_c, out, d_subs, d_desc, pl, plan, status, nonces, st_b, nn_b, st_c
                torch.cuda.empty_cache()
    return rows


def engine_leg(args, _lib, length, routings, knob=b"fanin_short", counter="fanin_frames"):
    """One sender engine produces every round's wire (--engine-frames publishes of `length` bytes to --engine-conns
    connections); one receiving engine per routing takes the same bytes; wall clock of flush_in.  routings:
    {name: the knob's value, or None to leave the knob alone (a library without it)}; knob: b"fanin_short", or
    b"fanin_split" with counter "fanin_split_frames"."""
    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    nc, nf = args.engine_conns, args.engine_frames
    precoms = [np.random.default_rng(1000 + i).integers(0, 256, size=32, dtype=np.uint8).tobytes() for i in range(nc)]
    tx = CurveBatchEngine(arena_bytes=nf * round_up(length, 16) + 4096)
    tx_ids = tx.add_connections(precoms, as_server=False)
    rxs = {k: CurveBatchEngine(arena_bytes=1 << 16) for k in routings}
    rx_ids = {k: e.add_connections(precoms, as_server=True) for k, e in rxs.items()}
    payloads = [np.random.default_rng(m).integers(0, 256, size=length, dtype=np.uint8).tobytes() for m in range(nf)]
    res = {k: [] for k in routings}
    routed = {k: 0 for k in routings}
    for rep in range(args.reps + 1):
        for p in payloads:
            tx.publish(tx_ids, p)
        tx.flush_out()
        wires = [tx.wire_out(c) for c in tx_ids]
        for k, short in routings.items():
            e = rxs[k]
            for c, w in zip(rx_ids[k], wires):
                e.recv(c, w)
            old = L.cz_tune(knob, short) if short is not None else None
            try:
                t0 = time.perf_counter()
                e.flush_in()
                t = time.perf_counter() - t0
            finally:
                if short is not None:
                    L.cz_tune(knob, old)
            if rep:
                res[k].append(t)
            if short is not None:
                routed[k] = getattr(e, counter)
            assert len(e.messages_in(rx_ids[k][0])) == nf and e.error(rx_ids[k][nc - 1]) == (0, 0)
    tx.close()
    for e in rxs.values():
        e.close()
    body = length + 33
    out = {"connections": nc, "frames_per_connection": nf, "len": length,
           "wire_bytes": nc * nf * (body + (9 if body > 255 else 2)), "clock": "time.perf_counter"}
    for k, v in res.items():
        out[k + "_flush_ms"] = round(statistics.median(v) * 1e3, 3)
        out[k + "_flush_all_ms"] = [round(t * 1e3, 3) for t in v]
        if routings[k] is not None:
            out[k + "_" + counter] = routed[k]
    return out


def split_rows(args, torch, dev, batch, _lib):
    """the device legs of --split: (e) cz_open_fanin_split, (a) cz_open_fanin_runs, (b) cz_open_segments"""
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for length in args.lens:
        size = length + 33
        bstride, pstride = round_up(size, 128), round_up(max(length, 1), 128)
        for nr, n in args.shapes:
            if nr * n * (bstride + pstride) > args.max_bytes:
                continue
            total = nr * n
            keys = torch.empty(n * 32, dtype=torch.uint8, device=dev)
            batch.fill(keys, 3)
            keys = keys.view(n, 32)
            payload = torch.empty(nr * round_up(length, 16) + 256, dtype=torch.uint8, device=dev)
            batch.fill(payload, 1)
            bodies = torch.zeros(total * bstride, dtype=torch.uint8, device=dev)
            out = torch.empty(total * pstride, dtype=torch.uint8, device=dev)
            rng = np.random.default_rng(total + length)
            base = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
            # the bodies: run r = one payload sealed for the n connections, counter base + r + 1
            ssubs = np.zeros(total, dtype=batch.FANOUT_SUB_DTYPE)
            ssubs["counter"] = (np.tile(base, nr) + np.repeat(np.arange(1, nr + 1, dtype=np.uint64), n))
            ssubs["key_idx"] = np.tile(np.arange(n), nr)
            sruns = np.zeros(nr, dtype=batch.FANOUT_RUN_DTYPE)
            sruns["payload_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(round_up(length, 16))
            sruns["out_off"] = np.arange(nr, dtype=np.uint64) * np.uint64(n * bstride)
            sruns["out_stride"], sruns["len"], sruns["count"] = bstride, length, n
            sruns["first_sub"] = np.arange(nr) * n
            splan = batch.plan_fanout(sruns, payload, bodies).to(dev)
            batch.seal_fanout_runs(splan, payload, torch.from_numpy(ssubs.view(np.uint8).copy()).to(dev), keys, bodies)
            del splan
            subs = np.zeros(total, dtype=batch.FANIN_SUB_DTYPE)
            subs["key_idx"] = ssubs["key_idx"]
            subs["flags"] = batch.FANIN_CHECK_NONCE | batch.FANIN_FLOOR_IS_BODY
            subs["floor"] = (np.arange(total, dtype=np.uint64) - np.uint64(n)) * np.uint64(bstride)
            subs["floor"][:n], subs["flags"][:n] = base, batch.FANIN_CHECK_NONCE
            d_subs = torch.from_numpy(subs.view(np.uint8).copy()).to(dev)
            runs = np.zeros(nr, dtype=batch.FANIN_RUN_DTYPE)
            runs["in_off"], runs["out_off"] = sruns["out_off"], np.arange(nr, dtype=np.uint64) * np.uint64(n * pstride)
            runs["in_stride"], runs["out_stride"], runs["size"], runs["count"] = bstride, pstride, size, n
            runs["first_sub"] = np.arange(nr) * n
            wire = total * (size + (9 if size > 255 else 2))
            seg = args.seg_blocks or flush_seg_blocks(wire)
            # (e) the grid, (a) one lane per body
            t0 = time.perf_counter()
            plan = batch.plan_fanin_split(runs, bodies, out, seg_blocks=seg)
            t_plan = time.perf_counter() - t0
            plan.to(dev)
            work = torch.empty(max(plan.npart, 1) * 64, dtype=torch.uint8, device=dev)
            plan_a = batch.plan_fanin(runs, bodies, out).to(dev)
            st_e, st_a, st_b = (torch.zeros(total, dtype=torch.int16, device=dev) for _ in range(3))
            nn_e, nn_a, nn_b = (torch.zeros(total, dtype=torch.int64, device=dev) for _ in range(3))
            # (b) descriptors with the same chains, the same segment length
            desc = np.zeros(total, dtype=batch.DESC_DTYPE)
            desc["in_off"] = np.arange(total, dtype=np.uint64) * np.uint64(bstride)
            desc["out_off"] = np.arange(total, dtype=np.uint64) * np.uint64(pstride)
            desc["len"], desc["key_idx"], desc["flags"] = size, ssubs["key_idx"], 0x100
            desc["counter"] = np.tile(base, nr)
            desc["prev"] = np.arange(total, dtype=np.int64) - n
            desc["prev"][:n] = -1
            t0 = time.perf_counter()
            pl = batch.SegmentPlan(desc, open_=True, seg_blocks=seg)
            t_plan_b = time.perf_counter() - t0
            pl.to(dev)
            d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
            e_args = (plan.d_runs.data_ptr(), nr, plan.d_tiles.data_ptr(), (ctypes.c_uint32 * 2)(*plan.class_count),
                      plan.d_joins.data_ptr() if len(plan.joins) else None, len(plan.joins), bodies.data_ptr(),
                      d_subs.data_ptr(), keys.data_ptr(), out.data_ptr(), work.data_ptr(), st_e.data_ptr(),
                      nn_e.data_ptr(), stream)
            a_args = (plan_a.d_runs.data_ptr(), nr, plan_a.d_waves.data_ptr(), (ctypes.c_uint32 * 3)(*plan_a.class_count),
                      plan_a.region_stride, bodies.data_ptr(), d_subs.data_ptr(), keys.data_ptr(), out.data_ptr(),
                      st_a.data_ptr(), nn_a.data_ptr(), stream)
            open_split, open_runs = L.cz_open_fanin_split, L.cz_open_fanin_runs

            def split():
                if open_split(*e_args):
                    raise RuntimeError(_lib.last_error())

            def fanin():
                if open_runs(*a_args):
                    raise RuntimeError(_lib.last_error())

            batch.open_fanin_split(plan, bodies, d_subs, keys, out, st_e, nonces=nn_e, work=work, subs_np=subs)  # bounds, once
            legs = {"split": split, "fanin": fanin,
                    "segments": lambda: batch.open_segments(d_desc, pl, bodies, out, keys, st_b, nonces=nn_b)}
            # sanity at the timed shape: every leg accepts every body and writes the same plaintext
            legs["segments"]()
            want = out.clone()
            for k, st, nn in (("split", st_e, nn_e), ("fanin", st_a, nn_a)):
                out.zero_()
                legs[k]()
                torch.cuda.synchronize()
                assert int((st != st_b).sum()) == 0 and int((st.view(torch.uint8)[::2] != 0).sum()) == 0, \
                    k + ": statuses differ or a body was rejected"
                assert torch.equal(nn, nn_b), k + ": nonces differ"
                assert torch.equal(want.view(total, pstride)[:, :length], out.view(total, pstride)[:, :length]), \
                    k + " and cz_open_segments disagree"
            del want
            inner = {}
            for k, fn in legs.items():     # warm-up, and enough calls for a ~2 ms window
                inner[k] = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, fn, 1), 1e-3))))
            times = {k: [] for k in legs}
            for rep in range(args.reps):
                for k, fn in legs.items():
                    times[k].append(event_ms(torch, fn, inner[k]))
            row = {"runs": nr, "n": n, "lanes": total, "len": length, "size": size, "in_stride": bstride,
                   "out_stride": pstride, "seg_blocks": seg, "tiles": len(plan.tiles), "joins": len(plan.joins),
                   "npart": plan.npart, "class_count": plan.class_count, "segments": pl.nseg,
                   "split_plan_host_ms": round(t_plan * 1e3, 4), "segments_plan_host_ms": round(t_plan_b * 1e3, 4),
                   "split_metadata_bytes": int(runs.nbytes + plan.tiles.nbytes + plan.joins.nbytes + subs.nbytes),
                   "segments_metadata_bytes": int(desc.nbytes + pl.nseg * 16 + pl.ncomb * 16)}
            for k in legs:
                row[k + "_ms"] = round(statistics.median(times[k]), 5)
                row[k + "_all_ms"] = [round(t, 5) for t in times[k]]
                row[k + "_spread_ms"] = round(max(times[k]) - min(times[k]), 5)
                row[k + "_calls_per_window"] = inner[k]
            rows.append(row)
            print(f"R={nr} n={n} len={length} seg={seg}: " + ", ".join(f"{k} {row[k + '_ms']} ms" for k in legs),
                  file=sys.stderr)
            del keys, payload, bodies, out, d_subs, d_desc, pl, plan, plan_a, work, st_e, st_a, st_b, nn_e, nn_a, nn_b
            torch.cuda.empty_cache()
    return rows


def fanin_split_rule(rows, engines, engine_frames=SPLIT_ENGINE_FRAMES):
    """the smallest measured length L such that every measured length >= L passes the device legs at every
    R x N >= 1024 and the engine legs at every engine shape (a shape that was not measured does not pass); 0 if none"""
    verdict = {}
    for length in sorted({r["len"] for r in rows}):
        dev = [r for r in rows if r["len"] == length and r["lanes"] >= 1024]
        dev_ok = bool(dev) and all(r["split_ms"] <= r["segments_ms"] for r in dev)
        eng = [e for e in engines if e["len"] == length]
        eng_ok = ({e["frames_per_connection"] for e in eng} >= set(engine_frames)
                  and all(e["routed_flush_ms"] <= e["unrouted_flush_ms"] for e in eng))
        verdict[str(length)] = {"device": dev_ok, "engine": eng_ok}
    best = 0
    for length in sorted((int(k) for k in verdict), reverse=True):
        if not (verdict[str(length)]["device"] and verdict[str(length)]["engine"]):
            break
        best = length
    return verdict, best


def fanin_short_rule(rows, engines):
    verdict = {}
    for length in sorted({r["len"] for r in rows}):
        dev_ok = all(r["fanin_ms"] <= r["segments_ms"] for r in rows if r["len"] == length and r["lanes"] >= 1024)
        eng = [e for e in engines if e["len"] == length]
        eng_ok = bool(eng) and all(e["routed_flush_ms"] <= e["unrouted_flush_ms"] for e in eng)
        verdict[str(length)] = {"device": dev_ok, "engine": eng_ok if eng else None}
    best = 0
    for length in sorted(int(k) for k in verdict):
        if not (verdict[str(length)]["device"] and verdict[str(length)]["engine"]):
            break
        best = length
    return verdict, best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lens", type=int, nargs="*", default=list(LENS))
    ap.add_argument("--runs-r", type=int, nargs="*", default=list(RUNS_R))
    ap.add_argument("--runs-n", type=int, nargs="*", default=list(RUNS_N))
    ap.add_argument("--seg-blocks", type=int, default=0, help="segment length of leg (b) (default: flush_in's)")
    ap.add_argument("--max-bytes", type=int, default=96 << 30, help="skip device shapes whose slots exceed this")
    ap.add_argument("--engine-conns", type=int, default=1024)
    ap.add_argument("--engine-frames", type=int, default=16)
    ap.add_argument("--engine-lens", type=int, nargs="*", default=None)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-device", action="store_true", help="skip the device legs")
    ap.add_argument("--ab-lib", default=None, help="a build of the parent commit: its flush_in, timed in a child process")
    ap.add_argument("--ab-name", default=None, help="what the second build is (recorded in the JSON)")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--split", action="store_true", help="the split fan-in legs, into profiles/fanin/fanin_split.json")
    ap.add_argument("--shapes", type=str, nargs="*", default=None, help="--split: R x N device shapes, as RxN")
    ap.add_argument("--engine-frames-list", type=int, nargs="*", default=list(SPLIT_ENGINE_FRAMES),
                    help="--split: frames per connection of the engine legs")
    ap.add_argument("--merge", action="store_true", help="--split: keep the legs already in --out that this run does not repeat")
    args = ap.parse_args()
    if args.split and args.lens == list(LENS):
        args.lens = list(SPLIT_LENS)
    args.shapes = [tuple(int(v) for v in sh.lower().split("x")) for sh in args.shapes] if args.shapes else list(SPLIT_SHAPES)
    args.out = args.out or os.path.join(ROOT, "profiles", "fanin", "fanin_split.json" if args.split else "fanin.json")
    if args.engine_lens is None:
        args.engine_lens = args.lens
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from jeromq_amd import _lib, batch, build
    assert torch.cuda.is_available(), "fanin_bench needs a GPU"
    if args.ab_child:   # (this process loaded the --ab-lib build through CZ_LIB: the unrouted flush alone)
        print(json.dumps([engine_leg(args, _lib, length, {"parent": None}) for length in args.engine_lens]))
        return
    dev = torch.device("cuda:0")
    L = _lib.lib()
    if args.split:
        return main_split(args, torch, dev, _lib, batch, build)
    L.cz_tune(b"fanin_split", 0)   # these legs measure the fan-in call against the segment plan alone
    default = L.cz_tune(b"fanin_short", 0)
    L.cz_tune(b"fanin_short", default)
    out = {"device": torch.cuda.get_device_name(0), "library": L.cz_version().decode(),
           "fanin_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, KERNELS),
           "segment_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, ["k_open_segments", "k_open_combine"]),
           "reps": args.reps, "clock_device": "hipEvent (torch.cuda.Event), median", "fanin_short_default": default,
           "ab_lib": args.ab_name or args.ab_lib}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if not args.no_device:
        out["device_legs"] = device_rows(args, torch, dev, batch, _lib)
        write()
    if not args.no_engine:
        out["engine"] = []
        for length in args.engine_lens:
            out["engine"].append(engine_leg(args, _lib, length, {"routed": length, "unrouted": 0}))
            write()
        if args.ab_lib:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--reps", str(args.reps),
                                    "--engine-conns", str(args.engine_conns), "--engine-frames", str(args.engine_frames),
                                    "--engine-lens"] + [str(v) for v in args.engine_lens],
                                   env=dict(os.environ, CZ_LIB=os.path.abspath(args.ab_lib)), capture_output=True,
                                   text=True, timeout=600)
            if child.returncode:
                raise RuntimeError("the --ab-lib child failed:\n" + child.stderr[-2000:])
            for e, p in zip(out["engine"], json.loads(child.stdout.strip().splitlines()[-1])):
                e["parent_flush_ms"], e["parent_flush_all_ms"] = p["parent_flush_ms"], p["parent_flush_all_ms"]
    if "device_legs" in out and "engine" in out:
        out["fanin_short_verdict"], out["fanin_short_rule"] = fanin_short_rule(out["device_legs"], out["engine"])
    write()
    print(json.dumps(out))


def main_split(args, torch, dev, _lib, batch, build):
    L = _lib.lib()
    default = L.cz_tune(b"fanin_split", 0)
    L.cz_tune(b"fanin_split", default)
    out = {}
    if args.merge and os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    hashes = {"split_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, SPLIT_KERNELS),
              "fanin_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, KERNELS),
              "segment_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, ["k_open_segments", "k_open_combine"])}
    if any(out.get(k, v) != v for k, v in hashes.items()):
        raise RuntimeError("--merge: the legs in --out were measured on other kernels")
    out.update({"device": torch.cuda.get_device_name(0), "library": L.cz_version().decode(), **hashes, "reps": args.reps,
                "clock_device": "hipEvent (torch.cuda.Event), median", "fanin_split_default": default,
                "fanin_short": L.cz_tune(b"fanin_short", 100)})
    L.cz_tune(b"fanin_short", out["fanin_short"])

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if not args.no_device:
        new = split_rows(args, torch, dev, batch, _lib)
        done = {(r["len"], r["runs"], r["n"]) for r in new}
        out["split_legs"] = sorted([r for r in out.get("split_legs", []) if (r["len"], r["runs"], r["n"]) not in done] + new,
                                   key=lambda r: (r["len"], r["lanes"], r["runs"]))
        write()
    if not args.no_engine:
        for length in args.engine_lens:
            for nf in args.engine_frames_list:
                args.engine_frames = nf
                e = engine_leg(args, _lib, length, {"routed": length, "unrouted": 0}, knob=b"fanin_split",
                               counter="fanin_split_frames")
                e["flush_spread_ms"] = {k: round(max(e[k + "_flush_all_ms"]) - min(e[k + "_flush_all_ms"]), 3)
                                        for k in ("routed", "unrouted")}
                out["engine_split"] = sorted([x for x in out.get("engine_split", [])
                                              if (x["len"], x["frames_per_connection"]) != (length, nf)] + [e],
                                             key=lambda x: (x["len"], x["frames_per_connection"]))
                print(f"engine len={length} frames={nf}: routed {e['routed_flush_ms']} ms, unrouted {e['unrouted_flush_ms']} ms",
                      file=sys.stderr)
                write()
    if "split_legs" in out and "engine_split" in out:
        out["fanin_split_verdict"], out["fanin_split_rule"] = fanin_split_rule(out["split_legs"], out["engine_split"])
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
