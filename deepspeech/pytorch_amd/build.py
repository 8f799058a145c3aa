"""Builds libds2hip.so (all HIP kernels + the C ABI) for gfx950, in-tree.

    python -m deepspeech.pytorch_amd.build            # or __graft_entry__.build()

hipcc cross-compiles without a GPU; the .so travels to the GPU box with the repo snapshot (it is git-ignored).
"""
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libds2hip.so")
SOURCES = ["ds2_norm.hip", "ds2_gemm.hip", "ds2_gemm8.hip", "ds2_rnn.hip", "ds2_rnn_persist.hip", "ds2_rnn_persist_gru.hip",
           "ds2_rnn_persist_lstm.hip", "ds2_rnn_persist_rnn.hip", "ds2_conv.hip", "ds2_ctc.hip", "ds2_seqops.hip", "ds2_decode.hip",
           "ds2_beam.hip", "ds2_errors.hip", "ds2_optim.hip", "ds2_spect.hip", "ds2_waveaug.hip", "ds2_align.hip", "ds2_fc.hip", "ds2_stream.hip",
           "ds2_resample.hip", "ds2_endpoint.hip", "ds2_confidence.hip", "ds2_kws.hip", "ds2_reverb.hip", "ds2_mwer.hip"]
# the general persistent recurrent kernels: instantiation source -> its table in ds2_rnn_persist_widths.h; one object per row
INSTANCES = {"ds2_rnn_persist3_inst.hip": "DS2_PERSIST3_WIDTHS", "ds2_rnn_persist2_inst.hip": "DS2_PERSIST2_INSTANCES"}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-pass-failed"]
FLAGS += os.environ.get("DS2_EXTRA_HIPCC_FLAGS", "").split()


# ds2_rnn_persist_impl.h lands its fire-and-forget scalar loads (l2_touch) in one fixed SGPR; nothing else may name that register,
# because the write arrives asynchronously.  The device assembly of these sources (kept by -save-temps) is checked after every compile.
L2_SINK_SOURCES = ("ds2_rnn_persist_gru.hip", "ds2_rnn_persist_lstm.hip", "ds2_rnn_persist_rnn.hip")
L2_SINK = 101


def _l2_sink_misuse(obj):
    stem = os.path.splitext(obj)[0]
    asm = [f for f in glob.glob(stem + "*gfx950*.s")]
    if not asm:
        return ["no device assembly found next to %s (-save-temps=obj)" % obj]
    bad = []
    single = re.compile(r"\bs%d\b" % L2_SINK)
    rng = re.compile(r"\bs\[(\d+):(\d+)\]")
    for f in asm:
        for ln, line in enumerate(open(f), 1):
            code = line.split(";")[0]
            if not code.strip() or code.lstrip().startswith("."):
                continue
            hit = bool(single.search(code)) or any(int(a) <= L2_SINK <= int(b) for a, b in rng.findall(code))
            if hit and not re.match(r"\s*s_load_dword s%d, s\[\d+:\d+\], 0x0\s*$" % L2_SINK, code):
                bad.append("%s:%d: %s" % (os.path.basename(f), ln, code.strip()))
    return bad


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def _instance_rows(table):
    """The rows of an X-macro table of ds2_rnn_persist_widths.h: the arguments of every line `X(...)` of its #define."""
    text = open(os.path.join(CSRC, "ds2_rnn_persist_widths.h")).read()
    body = re.search(r"^#define %s\(X\)((?:.*\\\n)*.*\n)" % table, text, re.M).group(1)
    return [re.sub(r"\s", "", row) for row in re.findall(r"^\s*X\((.*?)\)\s*\\?$", body, re.M)]


def build(force=False, verbose=True, probe=False):
    """probe=True: the instrumented library for tools/probe_rnn_persist.py (-DDS2_PROBE: in-kernel cycle counters and the
    DS2_PERSIST_DBG work-skipping masks) as libds2hip_probe.so -- never loaded by the product."""
    return _build("_probe", ["-DDS2_PROBE"], force, verbose) if probe else _build("", [], force, verbose)


def build_variant(name, extra_flags, force=False, verbose=False):
    """A/B builds (tools/ab_variants.py): the same sources with extra compiler flags (-DDS2_L2_AHEAD=4, -DDS2_CHUNK=8, ...) as
    libds2hip_<name>.so next to the shipping library -- never loaded by the product."""
    assert name.isidentifier() and name not in ("probe",), name
    return _build("_" + name, extra_flags, force, verbose)


def _build(suffix, extra_flags, force, verbose):
    obj_dir, lib_path, flags = OBJ + suffix, LIB.replace(".so", suffix + ".so"), FLAGS + list(extra_flags)
    os.makedirs(obj_dir, exist_ok=True)
    headers = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "..", "..", "include", "ds2hip.h")]
    units = [(src, os.path.join(obj_dir, src.replace(".hip", ".o")), []) for src in SOURCES]
    units += [(src, os.path.join(obj_dir, "%s_%s.o" % (src.replace("_inst.hip", ""), re.sub(r"\W+", "_", row))), ["-DDS2_INST=" + row])
              for src, table in INSTANCES.items() for row in _instance_rows(table)]
    jobs = [(os.path.join(CSRC, src), o, defs) for src, o, defs in units if force or _stale(o, [os.path.join(CSRC, src)] + headers)]

    def cc(job):
        s, o, defs = job
        extra = ["-save-temps=obj"] if os.path.basename(s) in L2_SINK_SOURCES else []
        r = subprocess.run([HIPCC] + flags + defs + extra + ["-c", s, "-o", o], capture_output=True, text=True)
        out = r.stdout + r.stderr
        if extra:
            bad = _l2_sink_misuse(o) if r.returncode == 0 else []
            stem = os.path.splitext(o)[0]
            for f in glob.glob(stem + "-hip-*") + glob.glob(stem + "-host-*") + glob.glob(stem + ".hip-hip-*"):   # -save-temps by-products
                os.remove(f)
            if bad:
                os.remove(o)
                return s, 1, "%s: the L2-touch sink register is used outside the touches:\n%s" % (s, "\n".join(bad[:10]))
        return s, r.returncode, out

    with ThreadPoolExecutor(max_workers=8) as ex:
        for s, rc, out in ex.map(cc, jobs):
            if verbose and out.strip():
                print(out, file=sys.stderr)
            if rc != 0:
                raise RuntimeError("hipcc failed on %s\n%s" % (s, out))
    objs = [o for _, o, _ in units]
    if force or jobs or _stale(lib_path, objs):
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_path] + objs, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed\n" + r.stdout + r.stderr)
    return lib_path


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, probe="--probe" in sys.argv))
