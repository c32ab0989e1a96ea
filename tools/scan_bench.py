#!/usr/bin/env python3
"""Device V2 scan (cz_v2_scan / cz_v2_scan_emit, header section 7b) against the host parse it replaces.

(a) Device legs, C connections x F frames x len (C in --conns, F in --frames, len = payload bytes in --lens): every
    stream is F V2 frames of len + 33 bytes, the streams back to back in device memory (any byte alignment, as
    received bytes lie).  HIP events around enough back-to-back calls for a ~2 ms window, median of --reps windows
    after a warm-up, legs interleaved:
      scan   cz_v2_scan (k_v2_scan + k_v2_place) and cz_v2_scan_emit (descriptors): what the scanned flush runs
             between the H2D of the received bytes and the open;
      host   what flush_in does for the same streams on the host before anything can be launched: one cz_v2_parse
             per stream and the descriptor / item records of its `build` step (here: numpy, vectorised).  Wall
             clock, through the Python binding, so each stream also pays one ctypes call; `host_call_overhead_ms`
             is the same number of calls of cz_v2_header_size, to be subtracted by the reader.  The host leg reads
             ONE stream's bytes again and again (cache-warm): it flatters the host.
(b) The flush: wall clock of flush_in with scan_in = the bytes a connection holds against scan_in = 0 on two
    engines of this process fed the same wire, one warm-up round, median of --reps, legs interleaved; and with
    --ab-lib (a build of the parent commit) the same flush once more in a child process that loads that library
    (CZ_LIB).  Shapes: 1024 connections x 16 frames of 100, 256, 1024 and 4096 B (DESIGN.md section 4 "Fan-in
    open"), and bench.py's small_flush shape that reaches 64 connections, 64 x 1 x 4096 B.

The rule that sets the shipped scan_in (the one that set fanin_short): the largest measured per-connection byte count
at which the scanned flush is not slower in the median than the unscanned leg of the same process, at every measured
shape at or below it; 0 if the smallest one loses.

Writes profiles/scan/scan.json and prints it."""
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

CONNS = (64, 1024, 16384)
FRAMES = (1, 16, 256)
LENS = (100, 4096)
ENGINE_SHAPES = ((1024, 16, 100), (1024, 16, 256), (1024, 16, 1024), (1024, 16, 4096), (64, 1, 4096))
KERNELS = ["k_v2_scan", "k_v2_place", "k_v2_emit"]


def round_up(v, a):
    return (v + a - 1) // a * a


def event_ms(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def v2_header(size):
    return bytes([2]) + size.to_bytes(8, "big") if size > 255 else bytes([0, size])


def device_rows(args, torch, dev, wire, _lib):
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for length in args.lens:
        size = length + 33
        for nc in args.conns:
            for nf in args.frames:
                one = (v2_header(size) + bytes(size)) * nf
                if nc * len(one) > args.max_bytes:
                    continue
                total = nc * nf
                d_wire = torch.from_numpy(np.frombuffer(one, dtype=np.uint8).copy()).to(dev).repeat(nc)
                st = np.zeros(nc, dtype=wire.V2_STREAM_DTYPE)
                st["off"] = np.arange(nc, dtype=np.uint64) * np.uint64(len(one))
                st["len"], st["floor"], st["key_idx"] = len(one), 2, np.arange(nc)
                d_streams = wire.to_device(st, dev)
                d_res = torch.zeros(nc * 32, dtype=torch.uint8, device=dev)
                d_tot = torch.zeros(16, dtype=torch.uint8, device=dev)
                d_desc = torch.zeros(total * 40, dtype=torch.uint8, device=dev)
                scan_args = (d_streams.data_ptr(), nc, d_wire.data_ptr(), -1, 128, d_res.data_ptr(), d_tot.data_ptr(), stream)
                emit_args = (d_streams.data_ptr(), d_res.data_ptr(), nc, d_wire.data_ptr(), 128, None, d_desc.data_ptr(),
                             stream)

                def scan():
                    if L.cz_v2_scan(*scan_args) or L.cz_v2_scan_emit(*emit_args):
                        raise RuntimeError(_lib.last_error())

                # the host leg: one parse per stream, then the records of flush_in's build step
                hbuf = np.frombuffer(one, dtype=np.uint8).copy()
                frames = np.zeros(nf + 1, dtype=wire.V2_FRAME_DTYPE)
                nfr, used = ctypes.c_uint32(), ctypes.c_uint64()
                parse = L.cz_v2_parse
                p_args = (hbuf.ctypes.data, len(hbuf), -1, frames.ctypes.data, nf + 1, ctypes.byref(nfr), ctypes.byref(used))
                desc = np.zeros(total, dtype=[("in_off", "<u8"), ("out_off", "<u8"), ("len", "<u4"), ("key_idx", "<u4"),
                                              ("counter", "<u8"), ("flags", "<u4"), ("prev", "<i4")])
                items = np.zeros(total, dtype=wire.V2_ITEM_DTYPE)
                bslot, pslot = round_up(size, 128), round_up(max(length, 1), 128)

                def host():
                    for _ in range(nc):
                        parse(*p_args)
                    body = (np.repeat(st["off"], nf) + np.tile(frames["body_off"][:nf], nc))
                    idx = np.arange(total, dtype=np.uint64)
                    items["src_off"], items["dst_off"], items["size"] = body, idx * np.uint64(bslot), size
                    desc["in_off"], desc["out_off"], desc["len"] = items["dst_off"], idx * np.uint64(pslot), size
                    desc["key_idx"], desc["counter"], desc["flags"] = np.repeat(st["key_idx"], nf), 2, 0x100
                    desc["prev"] = np.arange(total, dtype=np.int64) - 1
                    desc["prev"][::nf] = -1

                def overhead():
                    f = L.cz_v2_header_size
                    for _ in range(nc):
                        f(size)

                # sanity at the timed shape: the device's descriptors name the bodies the host parse found
                scan()
                torch.cuda.synchronize()
                host()
                got = d_desc.cpu().numpy().view(desc.dtype)
                tot = d_tot.cpu().numpy().view(wire.V2_TOTALS_DTYPE)[0]
                assert nfr.value == nf and (int(tot["nframes"]), int(tot["slot_bytes"])) == (total, total * pslot)
                assert np.array_equal(got["in_off"], items["src_off"]) and np.array_equal(got["out_off"], desc["out_off"])
                assert np.array_equal(got["prev"], desc["prev"]) and np.array_equal(got["len"], desc["len"])
                inner = max(1, min(200, math.ceil(2.0 / max(event_ms(torch, scan, 1), 1e-3))))
                times = {"scan": [], "host": [], "host_call_overhead": []}
                for rep in range(args.reps):
                    times["scan"].append(event_ms(torch, scan, inner))
                    times["host"].append(wall_ms(host))
                    times["host_call_overhead"].append(wall_ms(overhead))
                row = {"connections": nc, "frames_per_connection": nf, "len": length, "frames": total,
                       "stream_bytes": len(one), "scan_calls_per_window": inner,
                       "scan_metadata_bytes": int(st.nbytes), "host_metadata_bytes": int(desc.nbytes + items.nbytes)}
                for k, v in times.items():
                    row[k + "_ms"] = round(statistics.median(v), 5)
                    row[k + "_all_ms"] = [round(t, 5) for t in v]
                rows.append(row)
                print(f"C={nc} F={nf} len={length}: scan {row['scan_ms']} ms, host {row['host_ms']} ms "
                      f"(calls alone {row['host_call_overhead_ms']} ms)", file=sys.stderr)
                del d_wire, d_streams, d_res, d_tot, d_desc
                torch.cuda.empty_cache()
    return rows


def engine_leg(args, _lib, nc, nf, length, legs):
    """One sender engine produces every round's wire (nf publishes of `length` bytes to nc connections); one
    receiving engine per leg takes the same bytes; wall clock of flush_in.  legs: {name: scan_in for that flush, or
    None to leave the knob alone (a library without it)}."""
    from jeromq_amd.engine import CurveBatchEngine
    L = _lib.lib()
    precoms = [np.random.default_rng(1000 + i).integers(0, 256, size=32, dtype=np.uint8).tobytes() for i in range(nc)]
    tx = CurveBatchEngine(arena_bytes=nf * round_up(length, 16) + 4096)
    tx_ids = tx.add_connections(precoms, as_server=False)
    rxs = {k: CurveBatchEngine(arena_bytes=1 << 16) for k in legs}
    rx_ids = {k: e.add_connections(precoms, as_server=True) for k, e in rxs.items()}
    payloads = [np.random.default_rng(m).integers(0, 256, size=length, dtype=np.uint8).tobytes() for m in range(nf)]
    res = {k: [] for k in legs}
    scanned = {k: 0 for k in legs}
    per_conn = 0
    for rep in range(args.reps + 1):
        for p in payloads:
            tx.publish(tx_ids, p)
        tx.flush_out()
        wires = [tx.wire_out(c) for c in tx_ids]
        per_conn = max(len(w) for w in wires)
        for k, knob in legs.items():
            e = rxs[k]
            for c, w in zip(rx_ids[k], wires):
                e.recv(c, w)
            old = L.cz_tune(b"scan_in", per_conn if knob else 0) if knob is not None else None
            try:
                t0 = time.perf_counter()
                e.flush_in()
                t = time.perf_counter() - t0
            finally:
                if knob is not None:
                    L.cz_tune(b"scan_in", old)
            if rep:
                res[k].append(t)
            if knob is not None:
                scanned[k] = e.scan_frames
            assert len(e.messages_in(rx_ids[k][0])) == nf and e.error(rx_ids[k][nc - 1]) == (0, 0)
    tx.close()
    for e in rxs.values():
        e.close()
    out = {"connections": nc, "frames_per_connection": nf, "len": length, "bytes_per_connection": per_conn,
           "wire_bytes": nc * per_conn, "clock": "time.perf_counter"}
    for k, v in res.items():
        out[k + "_flush_ms"] = round(statistics.median(v) * 1e3, 3)
        out[k + "_flush_all_ms"] = [round(t * 1e3, 3) for t in v]
        if legs[k] is not None:
            out[k + "_scan_frames"] = scanned[k]
    return out


def scan_in_rule(engines):
    """the largest measured per-connection byte count such that the scanned flush is not slower than the unscanned one
    at every measured shape at or below it; 0 if none"""
    verdict, best = {}, 0
    for e in sorted(engines, key=lambda e: e["bytes_per_connection"]):
        ok = e["scanned_flush_ms"] <= e["unscanned_flush_ms"]
        verdict[f"{e['connections']}x{e['frames_per_connection']}x{e['len']}"] = {
            "bytes_per_connection": e["bytes_per_connection"], "not_slower": ok}
    for e in sorted(engines, key=lambda e: e["bytes_per_connection"]):
        if e["scanned_flush_ms"] > e["unscanned_flush_ms"]:
            break
        best = e["bytes_per_connection"]
    return verdict, best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lens", type=int, nargs="*", default=list(LENS))
    ap.add_argument("--conns", type=int, nargs="*", default=list(CONNS))
    ap.add_argument("--frames", type=int, nargs="*", default=list(FRAMES))
    ap.add_argument("--max-bytes", type=int, default=4 << 30, help="skip device shapes whose wire exceeds this")
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-device", action="store_true", help="skip the device legs")
    ap.add_argument("--ab-lib", default=None, help="a build of the parent commit: its flush_in, timed in a child process")
    ap.add_argument("--ab-name", default=None, help="what the second build is (recorded in the JSON)")
    ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan", "scan.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    import torch
    from jeromq_amd import _lib, build, wire
    assert torch.cuda.is_available(), "scan_bench needs a GPU"
    if args.ab_child:   # (this process loaded the --ab-lib build through CZ_LIB: its flush alone, no knob)
        print(json.dumps([engine_leg(args, _lib, nc, nf, length, {"parent": None}) for nc, nf, length in ENGINE_SHAPES]))
        return
    dev = torch.device("cuda:0")
    L = _lib.lib()
    default = L.cz_tune(b"scan_in", 0)
    L.cz_tune(b"scan_in", default)
    out = {"device": torch.cuda.get_device_name(0), "library": L.cz_version().decode(),
           "scan_kernels_sha256": build.kernel_code_sha256(_lib.LIB_PATH, KERNELS),
           "open_kernel_sha256": build.kernel_code_sha256(_lib.LIB_PATH, ["k_open_desc"]),
           "reps": args.reps, "clock_device": "hipEvent (torch.cuda.Event), median", "scan_in_default": default,
           "ab_lib": args.ab_name or args.ab_lib}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if not args.no_device:
        out["device_legs"] = device_rows(args, torch, dev, wire, _lib)
        write()
    if not args.no_engine:
        out["engine"] = []
        for nc, nf, length in ENGINE_SHAPES:
            e = engine_leg(args, _lib, nc, nf, length, {"scanned": 1, "unscanned": 0})
            out["engine"].append(e)
            print(f"engine {nc} x {nf} x {length}: scanned {e['scanned_flush_ms']} ms, unscanned {e['unscanned_flush_ms']} ms",
                  file=sys.stderr)
            write()
        if args.ab_lib:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--reps", str(args.reps)],
                                   env=dict(os.environ, CZ_LIB=os.path.abspath(args.ab_lib)), capture_output=True,
                                   text=True, timeout=600)
            if child.returncode:
                raise RuntimeError("the --ab-lib child failed:\n" + child.stderr[-2000:])
            for e, p in zip(out["engine"], json.loads(child.stdout.strip().splitlines()[-1])):
                e["parent_flush_ms"], e["parent_flush_all_ms"] = p["parent_flush_ms"], p["parent_flush_all_ms"]
        out["scan_in_verdict"], out["scan_in_rule"] = scan_in_rule(out["engine"])
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
