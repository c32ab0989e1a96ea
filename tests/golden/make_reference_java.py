#!/usr/bin/env python3
"""Records what the Java text checks need to know about the JeroMQ sources the binding targets, so
that tests/test_java_patch.py and tests/test_jni_shim.py run without those sources:

  python tests/golden/make_reference_java.py <root of the JeroMQ checkout>   -> reference_java.json

No source text is stored.  Per file the checks read:
  * "members": which of the declarations the tests name (their NEED_* tables) the file holds;
for the two files jni/patches/jeromq-gpu-curve.patch changes, also
  * "line_sha": sha256 (first 12 hex digits) of every line, against which the test matches each
    hunk's context and removed lines at the hunk's own line numbers (a clean apply: no offset, no fuzz);
  * "counts": braces and parentheses outside comments and literals, for the balance check;
  * "anchors": the line numbers of the method declarations the tests slice the patched text by.
Run it again whenever a test names a new member or anchor, or the patch moves to other sources."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_java_patch as tp  # noqa: E402
import test_jni_shim as ts  # noqa: E402


def line_sha(line):
    return hashlib.sha256(line.encode()).hexdigest()[:12]


def main(root):
    base = os.path.join(root, "jeromq-core/src/main/java/zmq")
    need = {}
    for table in (tp.NEED_MEMBERS, ts.NEED_REFERENCE_API):
        for f, members in table.items():
            need.setdefault(f, [])
            need[f] += [m for m in members if m not in need[f]]
    files = {}
    for f, members in sorted(need.items()):
        text = open(os.path.join(base, f)).read()
        files[f] = {"members": [m for m in members if m in text]}
    for f in tp.FILES:
        rel = os.path.relpath(f, "jeromq-core/src/main/java/zmq")
        text = open(os.path.join(root, f)).read()
        lines = text.split("\n")
        code = tp._strip(text)
        entry = files.setdefault(rel, {"members": []})
        entry["line_sha"] = [line_sha(ln) for ln in lines]
        entry["counts"] = {ch: code.count(ch) for ch in "{}()"}
        anchors = {}
        for a in tp.ANCHORS.get(os.path.basename(f), []):
            hits = [i + 1 for i, ln in enumerate(lines) if a in ln]
            assert len(hits) == 1, (f, a, hits)
            anchors[str(hits[0])] = a
        entry["anchors"] = anchors
    out = {"generator": "tests/golden/make_reference_java.py", "files": files}
    with open(os.path.join(HERE, "reference_java.json"), "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
