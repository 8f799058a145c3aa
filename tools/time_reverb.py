"""Times the reverberation kernel (csrc/ds2_reverb.hip) and the front-end calls around it.  profiles/reverb_timing.md holds its
output.

    python tools/time_reverb.py kernel            # 32 clips of 12-15 s: ds2_reverb with synthetic banks of 2048 / 8192 / 16384 taps at
                                                  # rir_prob 1.0 and 0.5, a batch mixing 512- and 16384-tap responses, and
                                                  # torch.nn.functional.conv1d per clip on the same inputs (--no-conv1d leaves it out)
    python tools/time_reverb.py frontend          # the un-augmented front-end call and the tempo + gain + noise call on the same clips
                                                  # (--root PATH imports the package from another checkout: the parent commit's), and,
                                                  # where the checkout has it, the call with reverberation in the chain

Every timed section is WARM warm-up calls and then CALLS timed ones between device events on the launching stream (one launch per
call for the kernel sections, so the event time is the kernel's time plus one launch).  Multiply-adds are counted as the rule
states them, sum over the reverberated clips of L * K (the taps that fall in front of the clip's start included), and the share of
peak is 2 * that / time / 157.3e12 (the fp32 matrix peak of the MI355X)."""
import argparse
import json
import os
import sys
import time

WARM, CALLS = 3, 20
PEAK_FP32 = 157.3e12


def _timed(fn, warm=WARM, calls=CALLS):
    import numpy as np
    import torch
    ev, wall = [], []
    for i in range(warm + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(i)
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        if i >= warm:
            ev.append(a.elapsed_time(b) * 1e3)
            wall.append((t1 - t0) * 1e3 * 1e3)
    return dict(event_us_median=round(float(np.median(ev)), 2), event_us_min=round(float(np.min(ev)), 2),
                event_us_std=round(float(np.std(ev)), 2), host_us_median=round(float(np.median(wall)), 2), calls=len(ev))


def _clips():
    import numpy as np
    import torch
    rng = np.random.RandomState(0)
    lens = sorted((int(v * 16000) for v in rng.uniform(12.0, 15.0, size=32)), reverse=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    wav = 0.1 * torch.randn((32, lens[0]), device="cuda", generator=g)
    for n, L in enumerate(lens):
        wav[n, L:] = 0
    return wav, lens


def _conv1d_per_clip(wav, lens, bank, off, ln, pk):
    """the stock route: per reverberated clip one torch.nn.functional.conv1d over the clip padded with p zeros behind and K - 1 - p
    in front, the taps reversed (conv1d correlates).  Every clip is taken at the batch's row length, so that one tap count is one
    shape for the library; the rows' own lengths are 12-15 s of it.  Returns (run(i), outputs list)."""
    import torch
    import torch.nn.functional as F
    jobs = []
    for n, L in enumerate(lens):
        if off[n] < 0:
            continue
        K, p = int(ln[n]), int(pk[n])
        w = bank[int(off[n]):int(off[n]) + K].flip(0).reshape(1, 1, K).contiguous()
        x = F.pad(wav[n].reshape(1, 1, -1), (K - 1 - p, p)).contiguous()
        jobs.append((n, x, w))
    outs = [None] * len(jobs)

    def run(i):
        for j, (n, x, w) in enumerate(jobs):
            outs[j] = F.conv1d(x, w)
    return run, jobs, outs


def kernel(a):
    import numpy as np
    import torch
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd.augment import RirBank
    wav, lens = _clips()
    ns = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = torch.empty_like(wav)
    print(json.dumps({"mode": "kernel", "clips": 32, "audio_seconds": round(sum(lens) / 16000.0, 1), "samples": sum(lens),
                      "tile": ops.query("ds2_reverb_tile") if hasattr(ops, "query") else None}), flush=True)
    r = _timed(lambda i: ops.reverb(wav, ns, None, None, None, None, out=out))
    print(json.dumps({"section": "copy (null rir_off)", "ds2_reverb": r}), flush=True)

    def section(name, taps_of_clip, prob, conv1d):
        """taps_of_clip: the tap count of every clip's response; a clip is reverberated when its draw comes up under prob"""
        rng = np.random.default_rng(1)
        kinds = sorted(set(taps_of_clip))
        rt60s = [(k - 0.5) / 16000.0 for k in kinds] * 4                  # ceil(rt60 * 16000) = k taps
        bank = RirBank.synthetic(rt60s, rng, drr_db=3.0, max_taps=max(kinds))
        pick = np.random.RandomState(2)
        off, ln, pk = np.full(32, -1, np.int64), np.zeros(32, np.int32), np.zeros(32, np.int32)
        for n in range(32):
            wet = pick.binomial(1, prob)
            r = kinds.index(taps_of_clip[n]) + len(kinds) * int(pick.choice(4))
            if wet:
                off[n], ln[n], pk[n] = bank.offsets[r], bank.length(r), bank.peaks[r]
        macs = float(sum(L * int(k) for L, k in zip(lens, ln)))
        offd, lnd, pkd = (torch.from_numpy(v).cuda() for v in (off, ln, pk))
        r = _timed(lambda i: ops.reverb(wav, ns, bank.samples, offd, lnd, pkd, out=out))
        res = {"section": name, "rir_prob": prob, "reverberated_clips": int((off >= 0).sum()), "taps": {str(k): int((ln == k).sum()) for k in kinds},
               "multiply_adds": macs, "ds2_reverb": r, "tflops": round(2 * macs / (r["event_us_median"] * 1e-6) / 1e12, 2),
               "share_of_fp32_peak": round(2 * macs / (r["event_us_median"] * 1e-6) / PEAK_FP32, 4)}
        if conv1d:
            try:
                run, jobs, outs = _conv1d_per_clip(wav, lens, bank.samples, off, ln, pk)
                c = _timed(run, warm=1, calls=3)
                ours = out.clone()
                err = max(float((outs[j][0, 0, :lens[n]] - ours[n, :lens[n]]).abs().max()) for j, (n, _, _) in enumerate(jobs))
                res.update({"conv1d_per_clip": dict(c, launches=len(jobs)), "conv1d_over_ds2_reverb": round(c["event_us_median"] / r["event_us_median"], 2),
                            "max_abs_difference_to_conv1d": err})
            except Exception as e:                                        # the stock route failing is a result too; it is printed
                res["conv1d_per_clip"] = "failed: %s: %s" % (type(e).__name__, str(e)[:200])
        print(json.dumps(res), flush=True)

    for taps in (2048, 8192, 16384):
        for prob in (1.0, 0.5):
            section("%d taps" % taps, [taps] * 32, prob, not a.no_conv1d)
    section("512 and 16384 taps, alternating clips", [512 if n % 2 else 16384 for n in range(32)], 1.0, False)
    section("512 taps", [512] * 32, 1.0, False)


def frontend(a):
    import numpy as np
    import torch
    from deepspeech.pytorch_amd import augment, configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    wav, lens = _clips()
    rng = np.random.default_rng(3)
    noise = augment.NoiseBank.from_waveforms([rng.uniform(-0.3, 0.3, 16 * 16000).astype(np.float32) for _ in range(4)])
    res = {"mode": "frontend", "root": a.root, "clips": 32}
    fe = SpectrogramFrontEnd(configs.SpectConfig())
    res["plain"] = _timed(lambda i: fe(wav, lens))
    wa = augment.WaveAugment(speed_volume_perturb=True, noise_bank=noise, noise_prob=0.4)
    fe2 = SpectrogramFrontEnd(configs.SpectConfig(), wave_augment=wa, rng=np.random.default_rng(4))
    res["tempo_gain_noise"] = _timed(lambda i: fe2(wav, lens))
    if hasattr(augment, "RirBank"):
        rirs = augment.RirBank.synthetic([0.3, 0.5, 0.8, 1.0], np.random.default_rng(5), drr_db=3.0)
        wa3 = augment.WaveAugment(speed_volume_perturb=True, noise_bank=noise, noise_prob=0.4, rir_bank=rirs, rir_prob=0.5)
        fe3 = SpectrogramFrontEnd(configs.SpectConfig(), wave_augment=wa3, rng=np.random.default_rng(4))
        res["tempo_reverb_gain_noise"] = _timed(lambda i: fe3(wav, lens))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernel", "frontend"))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--no-conv1d", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    {"kernel": kernel, "frontend": frontend}[a.mode](a)


if __name__ == "__main__":
    main()
