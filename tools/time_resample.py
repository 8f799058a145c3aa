"""Times the resampler (csrc/ds2_resample.hip) next to what it feeds.  profiles/resample_timing.md holds its output.

    python tools/time_resample.py oneshot --rate 48000        # 32 clips of 12-15 s: ds2_resample, then the spectrogram call on its output
    python tools/time_resample.py oneshot --mixed 8000,16000,48000     # the same clips spread over the rates: ONE ds2_resample_mixed
                                                                       # launch, then the single-rate call per rate it replaces
    python tools/time_resample.py oneshot --speed [--rate 48000]       # three-way speed perturbation: the classes rate x 0.9 / 1 / 1.1
    python tools/time_resample.py stream [--rate 48000]       # SpectStream.feed, 8 slots, 0.2 s chunks (no --rate: the 16 kHz path)
    python tools/time_resample.py copy                        # device copy bandwidth (the HBM floor's yardstick)
    python tools/time_resample.py summarise DIR               # per-kernel table from a rocprofv3 --kernel-trace --output-format csv run

Every timed section is WARM warm-up iterations and then CALLS timed ones, each iteration launching the same kernels, so the
summary takes, per kernel name whose dispatch count is a multiple of WARM + CALLS, the dispatches of the last CALLS iterations.
Kernel times come from a profiler run of its own,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_resample.py oneshot --rate 48000

and the event / wall times printed by the run itself are the host's view of the same calls.  --root PATH imports the package from
another checkout (the parent commit's, for the 16 kHz stream figure)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

WARM, CALLS = 3, 20


def _timed(fn):
    import numpy as np
    import torch
    ev, wall = [], []
    for i in range(WARM + CALLS):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(i)
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        if i >= WARM:
            ev.append(a.elapsed_time(b) * 1e3)
            wall.append((t1 - t0) * 1e3 * 1e3)
    return dict(event_us_median=round(float(np.median(ev)), 2), event_us_std=round(float(np.std(ev)), 2),
                host_us_median=round(float(np.median(wall)), 2), calls=len(ev))


def oneshot(a):
    import numpy as np
    import torch
    from deepspeech.pytorch_amd import configs, ops
    from deepspeech.pytorch_amd.resample import Resampler
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    rs = Resampler(a.rate)
    rng = np.random.RandomState(0)
    lens = sorted((int(v * a.rate) for v in rng.uniform(12.0, 15.0, size=32)), reverse=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    wav = 0.1 * torch.randn((32, lens[0]), device="cuda", generator=g)
    ns = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ldo = rs.out_len(lens[0])
    out = torch.empty((32, ldo), dtype=torch.float32, device="cuda")
    taps = rs.taps_on(wav.device)
    res = {"mode": "oneshot", "rate": a.rate, "U": rs.up, "D": rs.down, "W": rs.half_width, "clips": 32,
           "audio_seconds": round(sum(lens) / a.rate, 1), "bytes_in": 4 * sum(lens), "bytes_out": 4 * sum(rs.out_len(n) for n in lens)}
    res["ds2_resample"] = _timed(lambda i: ops.resample(wav, ns, taps, rs.up, rs.down, rs.half_width, ldo, out=out))
    ns16 = [rs.out_len(n) for n in lens]
    fe = SpectrogramFrontEnd(configs.SpectConfig())
    res["spectrogram_on_its_output"] = _timed(lambda i: fe(out, ns16))
    print(json.dumps(res))


def mixed(a):
    """32 clips of 12-15 s, clip i at rates[i % len(rates)]: one mixed launch against one single-rate launch per rate other than
    16 kHz (a 16 kHz clip costs the single-rate path nothing: its rows are not touched)"""
    import numpy as np
    import torch
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.augment import speed_rate
    from deepspeech.pytorch_amd.resample import ResamplerBank
    rates = [speed_rate(a.rate or 16000, s) for s in (0.9, 1.0, 1.1)] if a.speed else [int(r) for r in a.mixed.split(",")]
    bank = ResamplerBank(rates)
    rng = np.random.RandomState(0)
    secs = sorted(rng.uniform(12.0, 15.0, size=32), reverse=True)
    rate_of = [rates[i % len(rates)] for i in range(32)]
    lens = [int(v * r) for v, r in zip(secs, rate_of)]
    g = torch.Generator(device="cuda").manual_seed(0)
    wav = 0.1 * torch.randn((32, max(lens)), device="cuda", generator=g)
    ns = torch.tensor(lens, dtype=torch.int32, device="cuda")
    cls = torch.tensor([bank.class_of[r] for r in rate_of], dtype=torch.int32, device="cuda")
    lens16 = [bank.out_len(n, r) for n, r in zip(lens, rate_of)]
    out = torch.empty((32, max(lens16)), dtype=torch.float32, device="cuda")
    classes_dev, taps = bank.on(wav.device)
    res = {"mode": "oneshot-speed" if a.speed else "oneshot-mixed", "rates": rates, "clips": 32,
           "clips_per_rate": {str(r): rate_of.count(r) for r in rates}, "audio_seconds": round(float(sum(secs)), 1),
           "bytes_in": 4 * sum(lens), "bytes_out": 4 * sum(lens16)}
    res["ds2_resample_mixed"] = _timed(lambda i: ops.resample_mixed(wav, ns, cls, bank.classes, classes_dev, taps, out.shape[1], out=out))
    groups = []
    for r in rates:
        rs, idx = bank.resampler(r), [i for i in range(32) if rate_of[i] == r]
        if rs.identity or not idx:
            continue
        n_r = [lens[i] for i in idx]
        groups.append((rs, wav[idx, :max(n_r)].contiguous(), torch.tensor(n_r, dtype=torch.int32, device="cuda"), rs.taps_on(wav.device),
                       torch.empty((len(idx), rs.out_len(max(n_r))), dtype=torch.float32, device="cuda")))

    def per_rate(i):
        for rs, w, n, t, o in groups:
            ops.resample(w, n, t, rs.up, rs.down, rs.half_width, o.shape[1], out=o)
    res["ds2_resample_per_rate"] = dict(_timed(per_rate), launches=len(groups))
    print(json.dumps(res))


def stream(a):
    import numpy as np
    import torch
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    rate = a.rate or 16000
    kw = {"input_rate": a.rate} if a.rate else {}                     # the parent commit's front-end has no such argument
    fe = SpectrogramFrontEnd(configs.SpectConfig(), normalize="running", **kw)
    S, n = 8, int(0.2 * rate)
    st = fe.stream(S, "cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    chunks = [0.1 * torch.randn((S, n), device="cuda", generator=g) for _ in range(WARM + CALLS)]
    res = {"mode": "stream", "rate": a.rate, "slots": S, "chunk_samples": n}
    res["SpectStream.feed"] = _timed(lambda i: st.feed(range(S), chunks[i], [n] * S))
    print(json.dumps(res))


def copy(a):
    import torch
    n = 64 << 20                                                      # 256 MiB each way
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    r = _timed(lambda i: dst.copy_(src))
    r["GB_per_s_read_plus_write"] = round(2 * 4 * n / (r["event_us_median"] * 1e-6) / 1e9, 1)
    print(json.dumps({"mode": "copy", "bytes_each_way": 4 * n, "copy": r}))


def summarise(a):
    import numpy as np
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    by = {}
    for row in csv.DictReader(open(files[0])):
        by.setdefault(row["Kernel_Name"], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    print("| kernel | calls per iteration | avg us | min us | max us | std us |")
    print("|---|---|---|---|---|---|")
    per_iter, other = np.zeros(CALLS), []
    for name, d in sorted(by.items(), key=lambda kv: kv[1][0][0]):
        d.sort()
        if len(d) % (WARM + CALLS):
            other.append("`%s` x %d" % (name[:60], len(d)))
            continue
        c = len(d) // (WARM + CALLS)
        us = np.array([(e - s) / 1e3 for s, e in d[WARM * c:]]).reshape(CALLS, c)
        if a.only and not any(k in name for k in a.only.split(",")):
            other.append("`%s` x %d (%.2f us avg)" % (name[:60], len(d), us.mean()))
            continue
        per_iter += us.sum(1)
        print("| `%s` | %d | %.2f | %.2f | %.2f | %.2f |" % (name[:90], c, us.mean(), us.min(), us.max(), us.std()))
    print("\nkernel time per iteration over %d iterations: mean %.2f us, median %.2f, min %.2f, max %.2f, std %.2f"
          % (CALLS, per_iter.mean(), np.median(per_iter), per_iter.min(), per_iter.max(), per_iter.std()))
    if other:
        print("\nnot in the table (set-up, or excluded by --only): " + "; ".join(other))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("oneshot", "stream", "copy", "summarise"))
    ap.add_argument("dir", nargs="?")
    ap.add_argument("--rate", type=int, default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--mixed", default=None, help="oneshot: comma-separated rates, clip i at rates[i %% len]")
    ap.add_argument("--speed", action="store_true", help="oneshot: the classes --rate (default 16000) x 0.9 / 1.0 / 1.1")
    ap.add_argument("--only", default=None, help="summarise: comma-separated substrings of the kernel names to keep")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    if a.mode == "oneshot" and (a.mixed or a.speed):
        return mixed(a)
    if a.mode == "oneshot" and not a.rate:
        raise SystemExit("oneshot needs --rate, --mixed or --speed")
    {"oneshot": oneshot, "stream": stream, "copy": copy, "summarise": summarise}[a.mode](a)


if __name__ == "__main__":
    main()
