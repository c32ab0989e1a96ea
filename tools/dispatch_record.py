#!/usr/bin/env python3
"""Record which kernels the launchers of cz_kernels.hip launch, without a GPU.

cz_kernels.hip is compiled host-only with tools/dispatch_record/shim.h force-included, which turns
every hipLaunchKernelGGL into a print of the kernel as spelled, the grid, the LDS bytes and the
arguments; tools/dispatch_record/driver.cpp calls the launchers over a grid of layouts, lengths,
counts and knob settings.  The kernel names are normalised (enum names to values, defaulted template
arguments filled in), so two spellings of one instantiation record the same text.

    python tools/dispatch_record.py [--csrc DIR] [-o FILE] [--relay | --relay-segments]

--relay records the relay launcher's grid (czk_relay_uniform) instead, --relay-segments the segmented
relay's (czk_relay_segments); the default grid, and with it the parent's record, holds neither.

tests/golden/dispatch_parent.txt is the record of the commit before the launchers were rebuilt on
cz_dispatch.h; tests/test_dispatch_record.py requires the working tree to record the same text.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tools", "dispatch_record")
CSRC = os.path.join(ROOT, "jeromq_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ENUMS = {"ST_DIRECT": "0", "ST_LINES": "1", "ST_REGION": "2", "ST_SHIFT": "3",
         "MODE_ZMQ": "0", "MODE_NACL": "1", "MODE_BOX": "2"}
# template arguments a spelling may leave to their defaults: kernel -> (argument count, defaults from the right)
DEFAULTS = {"k_seal_uniform": (3, ["0"]), "k_open_uniform": (3, ["16"])}


def normalise_kernel(spelled):
    """'(k_seal_uniform<ST_LINES, true>)' -> 'k_seal_uniform<1,true,0>'"""
    s = re.sub(r"[()\s]", "", spelled)
    m = re.fullmatch(r"(\w+)(?:<(.*)>)?", s)
    if not m:
        raise ValueError(f"kernel spelling not understood: {spelled!r}")
    name, args = m.group(1), m.group(2)
    if args is None:
        return name
    args = [ENUMS.get(a, a) for a in args.split(",")]
    if name in DEFAULTS:
        n, tail = DEFAULTS[name]
        args += tail[len(tail) - (n - len(args)):] if len(args) < n else []
    return f"{name}<{','.join(args)}>"


def normalise(text):
    out = []
    for ln in text.splitlines():
        if ln.startswith("  ") and " g=" in ln:
            k, rest = ln[2:].split(" g=", 1)
            ln = f"  {normalise_kernel(k)} g={rest}"
        out.append(ln)
    return "\n".join(out) + "\n"


def signatures(text):
    """the distinct normalised kernels of a record"""
    return {ln[2:].split(" g=", 1)[0] for ln in text.splitlines() if ln.startswith("  ") and " g=" in ln}


def record(csrc=CSRC, relay=False, relay_segments=False):
    """Build the recorder against `csrc`/cz_kernels.hip, run it (relay / relay_segments: over that
    launcher's grid instead of the default one), return the normalised record."""
    if relay and relay_segments:
        raise ValueError("one grid per record: relay or relay_segments")
    with tempfile.TemporaryDirectory(prefix="cz_dispatch_") as td:
        exe = os.path.join(td, "dispatch_record")
        cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-std=c++17", "-O1", "-w",
               "-I" + os.path.join(ROOT, "include"), "-o", exe,
               "-include", os.path.join(HERE, "shim.h"), "-x", "hip", os.path.join(csrc, "cz_kernels.hip"),
               os.path.join(HERE, "driver.cpp")]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr[-4000:]}")
        raw = subprocess.run([exe] + (["relay"] if relay else ["relay_segments"] if relay_segments else []), capture_output=True, text=True, check=True).stdout
    return normalise(raw)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=CSRC, help="the directory holding cz_kernels.hip (default: this tree's)")
    ap.add_argument("-o", "--output", help="write the record here instead of standard output")
    ap.add_argument("--relay", action="store_true", help="record the relay launcher's grid instead of the default one")
    ap.add_argument("--relay-segments", action="store_true",
                    help="record the segmented relay launcher's grid instead of the default one")
    a = ap.parse_args()
    text = record(a.csrc, a.relay, a.relay_segments)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
