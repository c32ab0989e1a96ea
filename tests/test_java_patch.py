"""The last hop of the Java integration: jni/patches/jeromq-gpu-curve.patch wires
GpuCurveIoHook into the reference's StreamEngine and Poller.

No JDK exists in this image, so the patch is checked as text against what tests/golden/reference_java.json
records of the reference sources (tests/golden/make_reference_java.py; no source text is stored): it
applies cleanly to StreamEngine.java and Poller.java -- every hunk's context and removed lines match the
recorded line hashes at the hunk's own line numbers, so no offset and no fuzz; every GpuCurveIoHook member the patched code calls exists in
jni/java/zmq/io/GpuCurveIoHook.java with that many parameters; every Sink method is implemented; the
reference members the patched code relies on exist; braces balance.  The reference file:line anchors:
StreamEngine.java:379-535 (inEvent / outEvent), :958-1005 (mechanismReady), :1052-1111 (pullAndEncode,
decodeAndPush), :1170-1207 (heartbeats); Poller.java:194-284 (the loop)."""
import hashlib
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "jni", "patches", "jeromq-gpu-curve.patch")
HOOK = os.path.join(ROOT, "jni", "java", "zmq", "io", "GpuCurveIoHook.java")
RECORD = os.path.join(ROOT, "tests", "golden", "reference_java.json")
JAVA_ROOT = "jeromq-core/src/main/java/zmq"
FILES = [JAVA_ROOT + "/io/StreamEngine.java", JAVA_ROOT + "/poll/Poller.java"]
# declarations outside the patch's hunks that the tests slice the patched text by (recorded with their
# line numbers; every other line outside a hunk is left empty in the text the tests see)
ANCHORS = {"StreamEngine.java": ["private void mechanismReady()", "private Msg producePingMessage()",
                                 "private Msg producePongMessage(", "private Msg nextHandshakeCommand()"]}


def _record():
    with open(RECORD) as f:
        return json.load(f)["files"]


def _hunks(path):
    """{file: [(old_start, [(tag, line)])]} of a unified diff"""
    out, cur = {}, None
    for ln in open(path).read().split("\n"):
        if ln.startswith("+++ "):
            cur = out.setdefault(ln.split()[1].split("/", 1)[1], [])
        elif ln.startswith("@@"):
            cur.append((int(re.match(r"@@ -(\d+)", ln).group(1)), []))
        elif cur and ln[:1] in (" ", "+", "-") and not ln.startswith("--- "):
            cur[-1][1].append((ln[0], ln[1:]))
    return out


def _strip(code):
    """Java without comments and string / char literals (for brace and call counting)."""
    code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    return re.sub(r"\"(?:\\.|[^\"\\])*\"|'(?:\\.|[^'\\])'", "\"\"", code)


@pytest.fixture(scope="module")
def patched():
    """The patched files as far as the repository knows them: the patch applied at its own line numbers
    to a text that holds the recorded anchors and nothing else.  Every context and removed line must
    hash to the recorded line at its position; the brace and parenthesis counts of the result are the
    recorded counts plus what the hunks add and remove."""
    record, hunks = _record(), _hunks(PATCH)
    assert sorted(hunks) == sorted(FILES)
    out = {}
    for f in FILES:
        rec = record[os.path.relpath(f, JAVA_ROOT)]
        sha = rec["line_sha"]
        old = [""] * len(sha)
        for ln, text in rec["anchors"].items():
            old[int(ln) - 1] = text
        new, pos, counts = [], 0, dict(rec["counts"])
        for start, body in hunks[f]:
            new += old[pos:start - 1]
            pos = start - 1
            for tag, line in body:
                if tag in " -":
                    assert pos < len(sha) and hashlib.sha256(line.encode()).hexdigest()[:12] == sha[pos], \
                        (f, pos + 1, line)
                    pos += 1
                if tag in " +":
                    new.append(line)
            for tag, sign in (("+", 1), ("-", -1)):
                code = _strip("\n".join(line for t, line in body if t == tag))
                for ch in counts:
                    counts[ch] += sign * code.count(ch)
        new += old[pos:]
        out[os.path.basename(f)] = {"text": "\n".join(new), "counts": counts}
    return out


def _args(code, start):
    """top-level argument count of the call whose '(' ends at code[start - 1]"""
    depth, i, n = 1, start, 0
    while depth:
        ch = code[i]
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 1
        i += 1
    return n + (1 if code[start:i - 1].strip() else 0)


def _hook_api():
    src = _strip(open(HOOK).read())
    api = {}
    for m in re.finditer(r"public (?:static )?[\w<>\[\]]+ (\w+)\(([^)]*)\)", src):
        api[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    sink = re.search(r"interface Sink\s*\{(.*?)\n    \}", src, re.S).group(1)
    sink_methods = dict((m.group(1), len([a for a in m.group(2).split(",") if a.strip()]))
                        for m in re.finditer(r"\b[\w<>\[\]]+ (\w+)\(([^)]*)\);", sink))
    return api, sink_methods


def test_patch_applies_cleanly_to_the_reference(patched):
    for name, got in patched.items():
        c = got["counts"]
        assert c["{"] == c["}"] and c["("] == c[")"], name


def test_patched_code_calls_only_hook_members_that_exist(patched):
    api, sink = _hook_api()
    calls = 0
    for name, got in patched.items():
        code = _strip(got["text"])
        for m in re.finditer(r"\b(gpuHook|gpuCurve)\.(\w+)\(", code):
            meth = m.group(2)
            assert meth in api, (name, meth)
            assert _args(code, m.end()) == api[meth], (name, meth)
            calls += 1
        for m in re.finditer(r"\bGpuCurveIoHook\.([a-z]\w*)\(", code):   # static calls (not Sink)
            assert m.group(1) in api and _args(code, m.end()) == api[m.group(1)], (name, m.group(1))
            calls += 1
    se = _strip(patched["StreamEngine.java"]["text"])
    po = _strip(patched["Poller.java"]["text"])
    # the wiring the hook's header describes: attach at READY, hand over the decoder's leftover bytes,
    # delegate both events, resume after back-pressure, detach on teardown; one endOfLoop per iteration
    for must in ("gpuHook.attach(mechanism, gpuSink, fd)", "gpuHook.detach(gpuConn)", "gpuHook.outEvent(gpuConn)",
                 "gpuHook.inEvent(gpuConn, fd)", "gpuHook.handOver(gpuConn, inpos, insize)", "gpuHook.resume(gpuConn)",
                 "gpuHook.writeBacklog(gpuConn)", "ioThread.getPoller().gpuCurveHook()"):
        assert must in se, must
    for must in ("GpuCurveIoHook.fromSystemProperties()", "gpuCurve.endOfLoop()", "gpuCurve.close()"):
        assert must in po, must
    assert po.count("flushGpuCurve();") == 2       # after the handlers, and on a select timeout
    assert calls >= 11
    # every Sink method is implemented by the patched StreamEngine, with its parameter count
    body = se[se.index("new GpuCurveIoHook.Sink()"):]
    for meth, n in sink.items():
        m = re.search(r"public [\w<>\[\]]+ " + meth + r"\(([^)]*)\)", body)
        assert m, meth
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n, meth


def test_attached_connections_never_reach_the_cpu_mechanism(patched):
    """After attach the mechanism's nonce counters belong to the engine: no encode / decode may run on
    the CPU -- pullAndEncode is swapped for the plain session pull, heartbeats are left plaintext for
    the hook, the first inbound message skips mechanism.decode, and back-pressure never returns to
    decodeAndPush."""
    se = _strip(patched["StreamEngine.java"]["text"])
    ready = se[se.index("private void mechanismReady()"):se.index("new GpuCurveIoHook.Sink()")]
    assert "nextMsg = pullMsgFromSession;" in ready.split("gpuHook.attach(")[1]
    for fn in ("private Msg producePingMessage()", "private Msg producePongMessage("):
        body = se[se.index(fn):]
        body = body[:body.index("return msg;")]
        assert "if (gpuConn < 0) {\n            msg = mechanism.encode(msg);" in body, fn
        assert "nextMsg = gpuConn >= 0 ? pullMsgFromSession : pullAndEncode;" in body, fn
    assert "processMsg = gpuConn >= 0 ? pushDecoded : decodeAndPush;" in se
    assert "if (errno.is(ZError.EAGAIN) && gpuConn < 0) {\n                processMsg = pushOneThenDecodeAndPush;" in se
    hs = se[se.index("private Msg nextHandshakeCommand()"):]
    hs = hs[:hs.index("return pullAndEncode.get();")]
    assert "gpuHook.outEvent(gpuConn);\n                return null;" in hs


def test_reference_members_the_patch_relies_on_exist():
    """as recorded from the reference's text (tests/golden/reference_java.json): never built or run here"""
    record = _record()
    for f, members in NEED_MEMBERS.items():
        for m in members:
            assert m in record[f]["members"], (f, m)


NEED_MEMBERS = {
        "io/IOThread.java": ["Poller getPoller()"],
        "io/IOObject.java": ["public final void setPollIn(Handle handle)", "public final void setPollOut(Handle handle)",
                             "public final void resetPollIn(Handle handle)", "public final void resetPollOut(Handle handle)"],
        "io/SessionBase.java": ["public void flush()"],
        "util/Errno.java": ["public boolean is(int err)"],
        "Options.java": ["public Mechanisms mechanism"],
        "io/mechanism/Mechanisms.java": ["CURVE"],
        "SocketBase.java": ["public final void eventHandshakeFailedProtocol(String addr, int errno)"],
        "poll/PollerBase.java": ["protected final Thread worker;"],
        "io/StreamEngine.java": ["private SocketChannel fd;", "private ByteBuffer inpos;", "private int insize;",
                                 "private int outsize;", "private boolean plugged;", "private Supplier<Msg> nextMsg;",
                                 "private Function<Msg, Boolean> processMsg;", "private boolean inputStopped;",
                                 "private boolean outputStopped;", "private void error(ErrorReason error)",
                                 "private final Supplier<Msg> pullMsgFromSession"],
        "poll/Poller.java": ["private final UncaughtExceptionHandler exnotification;"],
}
