#!/usr/bin/env python
"""Chunked batch-1 inference with hidden-state carry -- reference inference.py:79-99 (run_transcribe: eval mode, one utterance,
`hs` fed back chunk after chunk, outputs concatenated on the time axis) -- on the drop-in class, and the same loop on stock
PyTorch-ROCm (oracle/ds2_torch_port.py).  SURVEY.md section 8(f)-4: the serving path reuses the training kernels (the persistent
forward sweep takes h0/c0 and returns hn/cn).  Prints one JSON line per model: per-chunk latency and real-time factor.

    python tools/bench_stream.py [--seconds 30 --chunk 2.0 --stock]
    python tools/bench_stream.py --decode beam [--beam-width 100]
    python tools/bench_stream.py --carry [--decode greedy --chunk 0.2 --streams 1]
    python tools/bench_stream.py --pool 8 [--chunk 0.2 --seconds 10 --pool-modes sessions,pool,session,pool_lockstep --pool-launches]
    python tools/bench_stream.py --carry --wave      /      --pool 8 --wave      [--rate 48000]
    python tools/bench_stream.py --pool 8 --wave --rates 8000,16000,48000     # one pool at mixed rates against one pool per rate

With --decode greedy|beam the drop-in class runs inside a streaming.StreamingTranscriber: every chunk's output goes to the decoder
stream on the device and the best transcript so far comes back per chunk (no output leaves the device, nothing is decoded twice).

--carry times a session feed of the uni-directional model in both modes at the same chunk size: the default one (every chunk on its
own, as in the reference) and carry_context=True (exact chunked inference: conv and lookahead context carried on the device, DESIGN.md
section 3.6.2); the exact mode ends the utterance with end().  It also prints, for a small uni-directional GRU in bf16, the error of
the streamed probabilities and of the one-shot forward against the fp64 oracle (e_stream, e_oneshot).

--pool S times one TICK of S exact streams of the uni-directional model, a tick being one chunk for every open stream, stream k
joining at tick k, in four modes: `sessions`, S StreamingTranscriber(carry_context=True) sessions of one
stream each, fed one after another (the only way to serve staggered streams without a pool); `pool`, one StreamPool feed per tick;
and, with all streams joining at tick 0, `session` (one lock-step session of S streams) against `pool_lockstep`.  Only the ticks
in which all S streams are open and none ends are timed.  --pool-launches adds the device kernels of one such tick (torch.profiler).

--wave (with --carry or --pool): the exact modes are fed raw audio, feed_wave instead of feed, in the same chunking (chunk seconds
* 16000 samples a feed): the streaming front-end with running normalisation runs inside the timed feed.
--rate R (with --wave): the audio arrives at R Hz, chunk seconds * R samples a feed, and the front-end is built with input_rate=R,
so the resampler runs inside the timed feed as well.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def run(model_fn, chunks, reps):
    lat = []
    for r in range(reps + 1):
        hs, outs = None, []
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for c in chunks:
            t0 = time.perf_counter()
            out, hs = model_fn(c, hs)
            outs.append(out.cpu())              # as run_transcribe does: every chunk's output leaves the device
            if r > 0:
                lat.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        total = time.perf_counter() - t_all
    return np.array(lat), total, torch.cat(outs, 1)


def run_decoding(st, chunks, reps):
    """run() through a StreamingTranscriber: per-chunk latency includes the decoder feed and the fetch of the best transcript"""
    lat = []
    for r in range(reps + 1):
        st.reset()
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for c in chunks:
            t0 = time.perf_counter()
            text = st.feed(c, torch.tensor([c.shape[3]], dtype=torch.int))
            if r > 0:
                lat.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        total = time.perf_counter() - t_all
    return np.array(lat), total, text, st.frames


def run_carry(st, chunks, reps, N, wave=False):
    """run_decoding() for either mode of a session over N streams; the exact mode ends the utterance (end()) outside the timed feeds"""
    lat, emitted = [], 0
    for r in range(reps + 1):
        st.reset()
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for c in chunks:
            t0 = time.perf_counter()
            text = st.feed_wave(c, [c.shape[1]] * N) if wave else st.feed(c, [c.shape[3]] * N)
            if r > 0:
                lat.append(time.perf_counter() - t0)
        emitted = st.frames[0]
        if st.carry_context:
            text = st.end()
        torch.cuda.synchronize()
        total = time.perf_counter() - t_all
    return np.array(lat), total, text, emitted, st.frames[0]


def carry_error():
    """bf16 on a small uni-directional GRU (32 units, 2 layers, lookahead 20), 2 streams of 160 / 155 frames fed as (54, 1, 2, 37, 66):
    max |p - p_oracle| over the valid frames of the streamed session and of the one-shot forward"""
    from deepspeech.pytorch_amd import configs, decoder as D, synth
    from deepspeech.pytorch_amd.model import DeepSpeech
    from deepspeech.pytorch_amd.streaming import StreamingTranscriber
    from oracle import ds2_oracle as O, ds2_torch_port as TP
    cfg = dict(rnn_type="gru", hidden_size=32, hidden_layers=2, bidirectional=False, lookahead_context=20)
    state = TP.random_state(cfg, 0)
    mc = configs.UniDirectionalConfig(rnn_type=configs.RNNType.gru, hidden_size=32, hidden_layers=2, lookahead_context=20)
    m = DeepSpeech(configs.LABELS, mc, "bf16", configs.AdamConfig(), configs.SpectConfig())
    m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
    m = m.to("cuda").eval()
    lengths = np.array([160, 155])
    inputs = synth.synth_batch(lengths, seed=11)[0]
    P = {k: v.double().numpy() if v.dtype.is_floating_point else v.numpy() for k, v in state.items()}
    ref, out_lens = O.model_forward(P, cfg, inputs.astype(np.float64), lengths, train=False, keep_cache=False)[:2]
    x = torch.from_numpy(inputs).to("cuda")
    with torch.no_grad():
        one = m(x, torch.from_numpy(lengths).int())[0].double().cpu().numpy()
    st = StreamingTranscriber(m, D.GreedyDecoder(configs.LABELS), carry_context=True)
    got, pos, chunks = [[], []], 0, (54, 1, 2, 37, 66)
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        st.feed(x[:, :, :, pos:pos + c].contiguous(), [int(g) - pos for g in lengths] if last else [c, c], final=last)
        if st.last_output is not None:
            for n in range(2):
                got[n].append(st.last_output[0][n, :st.last_output[1][n]].double().cpu().numpy())
        pos += c
    err = lambda rows: float(max(np.abs(rows[n] - ref[n, :out_lens[n]]).max() for n in range(2)))
    print(json.dumps({"metric": "bf16 probabilities against the fp64 oracle, max abs over valid frames", "model": "uni-GRU-32x2+lookahead20",
                      "frames": lengths.tolist(), "chunks": list(chunks), "e_stream": err([np.concatenate(g) for g in got]),
                      "e_oneshot": err([one[n, :out_lens[n]] for n in range(2)])}))


def _uni_lstm(dev):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.model import DeepSpeech
    from oracle import ds2_torch_port as TP
    cfg = dict(rnn_type="lstm", hidden_size=1024, hidden_layers=5, bidirectional=False, lookahead_context=20)
    mc = configs.UniDirectionalConfig(rnn_type=configs.RNNType.lstm, hidden_size=1024, hidden_layers=5, lookahead_context=20)
    m = DeepSpeech(configs.LABELS, mc, "bf16", configs.AdamConfig(), configs.SpectConfig())
    m.load_state_dict({k: v.clone() for k, v in TP.random_state(cfg, 0).items()}, strict=True)
    return m.to(dev).eval()


def _front_end(a):
    """--rate: a causal front-end that takes the audio at that rate; None = the sessions make their own 16 kHz one"""
    if not a.rate:
        return None
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    return SpectrogramFrontEnd(configs.SpectConfig(), normalize="running", input_rate=a.rate)


def run_pool(a):
    """--pool: see the module docstring.  One JSON line per mode."""
    from deepspeech.pytorch_amd import configs, decoder as D, streaming
    dev, S, tc = "cuda", a.pool, int(a.chunk * 100)
    nch = int(a.seconds * 100) // tc
    m = _uni_lstm(dev)
    mk_dec = lambda: D.BeamCTCDecoder(configs.LABELS, beam_width=a.beam_width) if a.decode == "beam" else D.GreedyDecoder(configs.LABELS)
    spc = int(round(a.chunk * (a.rate or 16000)))           # samples a wave feed brings per stream
    if a.wave:
        audio = torch.from_numpy(0.1 * np.random.RandomState(0).standard_normal((S, nch * spc)).astype(np.float32)).to(dev)
        piece = lambda k, j: audio[k:k + 1, j * spc:(j + 1) * spc]
    else:
        audio = torch.from_numpy(np.random.RandomState(0).standard_normal((S, 1, 161, nch * tc)).astype(np.float32)).to(dev)
        piece = lambda k, j: audio[k:k + 1, :, :, j * tc:(j + 1) * tc]
    per = spc if a.wave else tc                           # what a feed brings per stream: samples or frames
    feed_of = lambda obj: obj.feed_wave if a.wave else obj.feed
    max_frames = nch * tc // 2 + 2
    # --endpoint: decoder.Endpointer's default rule (a segment no longer than the pool that the other runs get)
    ep = D.Endpointer(max_segment=min(1000, max_frames)) if a.endpoint else None

    def ticks_of(starts):
        """per tick the streams that are open, (stream, its chunk index), and whether the tick is timed"""
        out = []
        for t in range(max(starts) + nch):
            rows = [(k, t - starts[k]) for k in range(S) if 0 <= t - starts[k] < nch]
            out.append((rows, len(rows) == S and all(j < nch - 1 for _, j in rows)))
        return out

    def measure(mode):
        starts = list(range(S)) if mode in ("sessions", "pool") else [0] * S
        plan = ticks_of(starts)
        batches = [torch.cat([piece(k, j) for k, j in rows]).contiguous() for rows, _ in plan]      # the caller's batch, not timed
        if mode == "sessions":
            sess = [streaming.StreamingTranscriber(m, mk_dec(), front_end=_front_end(a), max_frames=max_frames, carry_context=True,
                                                     endpoint=ep) for _ in range(S)]
            xs = [[piece(k, j).contiguous() for k, j in rows] for rows, _ in plan]
        elif mode == "session":
            sess = streaming.StreamingTranscriber(m, mk_dec(), front_end=_front_end(a), max_frames=max_frames, carry_context=True,
                                                  endpoint=ep)
        else:
            pool = streaming.StreamPool(m, mk_dec(), S, max_frames=max_frames, front_end=_front_end(a), endpoint=ep)
        lat, launches = [], None
        for r in range(a.reps + 1 + int(a.pool_launches)):
            if mode == "sessions":
                for st in sess:
                    st.reset()
            elif mode == "session":
                sess.reset()
            else:
                slot = {}
            prof_tick = next(i for i, (_, timed) in enumerate(plan) if timed) + 2 if a.pool_launches and r == a.reps + 1 else -1
            for i, (rows, timed) in enumerate(plan):
                if i == prof_tick:
                    prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA])
                    prof.__enter__()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "sessions":
                    for x, (k, j) in zip(xs[i], rows):
                        feed_of(sess[k])(x, [per], final=(j == nch - 1))
                elif mode == "session":
                    feed_of(sess)(batches[i], [per] * S, final=(rows[0][1] == nch - 1))
                else:
                    for k, j in rows:
                        if j == 0:
                            slot[k] = pool.open()
                    feed_of(pool)([slot[k] for k, _ in rows], batches[i], [per] * len(rows), final=[slot[k] for k, j in rows if j == nch - 1])
                    for k, j in rows:
                        if j == nch - 1:
                            pool.close(slot[k])
                torch.cuda.synchronize()
                if i == prof_tick:
                    prof.__exit__(None, None, None)
                    launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
                elif timed and 0 < r <= a.reps:
                    lat.append(time.perf_counter() - t0)
        lat = np.array(lat)
        print(json.dumps({"metric": "one tick of S exact streams (every open stream advances one chunk)", "mode": mode, "streams": S,
                          "model": "uni-LSTM-1024x5+lookahead", "decode": a.decode or "greedy", "input": "wave" if a.wave else "spectrogram",
                          "input_rate": (a.rate or 16000) if a.wave else None,
                          "chunk_seconds": a.chunk, "endpoint": repr(ep) if ep is not None else None,
                          "chunks_per_stream": nch, "ticks_timed": int(lat.size), "ms_per_tick_median": round(float(np.median(lat)) * 1e3, 3),
                          "ms_per_tick_p95": round(float(np.percentile(lat, 95)) * 1e3, 3), "device_kernels_per_tick": launches,
                          "dtype": "bf16"}), flush=True)

    for mode in a.pool_modes.split(","):
        if mode not in ("sessions", "pool", "session", "pool_lockstep"):
            raise SystemExit("unknown --pool-modes entry %r" % mode)
        measure(mode)


def run_pool_rates(a):
    """--pool S --wave --rates R1,R2,...: stream k arrives at rates[k % len(rates)] and joins at tick k.  `pool_mixed` is ONE
    StreamPool of S slots whose front-end takes the set of rates (open(rate=...)): one feed_wave per tick.  `pool_per_rate` is
    what a single-rate front-end leaves: one StreamPool per rate, each fed once per tick.  Only the ticks in which all S streams
    are open and none ends are timed.  One JSON line per mode."""
    from deepspeech.pytorch_amd import configs, decoder as D, streaming
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    dev, S, tc = "cuda", a.pool, int(a.chunk * 100)
    nch = int(a.seconds * 100) // tc
    rates = [int(r) for r in a.rates.split(",")]
    rate_of = [rates[k % len(rates)] for k in range(S)]
    spc = [int(round(a.chunk * r)) for r in rate_of]
    m = _uni_lstm(dev)
    rng = np.random.RandomState(0)
    audio = [torch.from_numpy(0.1 * rng.standard_normal(nch * n).astype(np.float32)).to(dev) for n in spc]
    max_frames = nch * tc // 2 + 2
    fe_of = lambda r: SpectrogramFrontEnd(configs.SpectConfig(), normalize="running", input_rate=r)
    plan = []
    for t in range(S - 1 + nch):
        rows = [(k, t - k) for k in range(S) if 0 <= t - k < nch]
        plan.append((rows, len(rows) == S and all(j < nch - 1 for _, j in rows)))

    def batch(rows):
        if not rows:                      # a pool none of whose streams is open in this tick
            return None
        buf =torch.zeros((len(rows), max(spc[k] for k, _ in rows)), device=dev)
        for i, (k, j) in enumerate(rows):
            buf[i, :spc[k]] = audio[k][j * spc[k]:(j + 1) * spc[k]]
        return buf

    def measure(mode):
        groups = [list(range(S))] if mode == "pool_mixed" else [[k for k in range(S) if rate_of[k] == r] for r in rates]
        groups = [g for g in groups if g]
        pools = [streaming.StreamPool(m, D.GreedyDecoder(configs.LABELS), len(g), max_frames=max_frames,
                                      front_end=fe_of(tuple(rates) if mode == "pool_mixed" else rate_of[g[0]])) for g in groups]
        feeds = [[(rows_g, batch(rows_g)) for rows_g in ([(k, j) for k, j in rows if k in g] for g in groups)] for rows, _ in plan]
        lat = []
        for r in range(a.reps + 1):
            slot = {}
            for i, (rows, timed) in enumerate(plan):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for pool, (rows_g, buf) in zip(pools, feeds[i]):
                    if not rows_g:
                        continue
                    for k, j in rows_g:
                        if j == 0:
                            slot[k] = pool.open(rate=rate_of[k]) if mode == "pool_mixed" else pool.open()
                    pool.feed_wave([slot[k] for k, _ in rows_g], buf, [spc[k] for k, _ in rows_g],
                                   final=[slot[k] for k, j in rows_g if j == nch - 1])
                    for k, j in rows_g:
                        if j == nch - 1:
                            pool.close(slot[k])
                torch.cuda.synchronize()
                if timed and r > 0:
                    lat.append(time.perf_counter() - t0)
        lat = np.array(lat)
        print(json.dumps({"metric": "one tick of S exact streams at mixed rates (every open stream advances one chunk)", "mode": mode,
                          "streams": S, "rates": rate_of, "pools": len(pools), "model": "uni-LSTM-1024x5+lookahead", "decode": "greedy",
                          "chunk_seconds": a.chunk, "chunks_per_stream": nch, "ticks_timed": int(lat.size),
                          "ms_per_tick_median": round(float(np.median(lat)) * 1e3, 3),
                          "ms_per_tick_p95": round(float(np.percentile(lat, 95)) * 1e3, 3), "dtype": "bf16"}), flush=True)

    for mode in ("pool_per_rate", "pool_mixed", "pool_per_rate", "pool_mixed"):
        measure(mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--chunk", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stock", action="store_true")
    ap.add_argument("--decode", choices=("greedy", "beam"), default=None, help="decode inside the chunk loop (StreamingTranscriber)")
    ap.add_argument("--beam-width", type=int, default=100)
    ap.add_argument("--carry", action="store_true", help="time a session feed with and without carry_context (uni-directional model)")
    ap.add_argument("--streams", type=int, default=1, help="--carry: streams fed in lock step")
    ap.add_argument("--pool", type=int, default=0, help="time one tick of this many exact streams (StreamPool and its baselines)")
    ap.add_argument("--pool-modes", default="sessions,pool,session,pool_lockstep")
    ap.add_argument("--pool-launches", action="store_true", help="--pool: also count the device kernels of one tick")
    ap.add_argument("--wave", action="store_true", help="--carry / --pool: feed raw audio (feed_wave) to the exact modes")
    ap.add_argument("--endpoint", action="store_true", help="--pool: the sessions and the pool cut their streams into utterances")
    ap.add_argument("--rate", type=int, default=None, help="--wave: the sample rate of the audio fed (the front-end's input_rate)")
    ap.add_argument("--rates", default=None, help="--pool --wave: comma-separated rates, stream k at rates[k %% len]: one pool at "
                                                  "mixed rates against one pool per rate")
    a = ap.parse_args()
    if a.wave and not (a.pool or a.carry):
        raise SystemExit("--wave goes with --carry or --pool")
    if a.endpoint and not a.pool:
        raise SystemExit("--endpoint goes with --pool")
    if a.rate and not a.wave:
        raise SystemExit("--rate goes with --wave")
    if a.rates and not (a.pool and a.wave) or a.rates and a.rate:
        raise SystemExit("--rates goes with --pool and --wave, and without --rate")
    if a.pool and a.rates:
        return run_pool_rates(a)
    if a.pool:
        return run_pool(a)
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.model import DeepSpeech
    from oracle import ds2_torch_port as TP
    dev = "cuda"
    T, tc = int(a.seconds * 100), int(a.chunk * 100)
    rs = np.random.RandomState(0)
    spect = torch.from_numpy(rs.standard_normal((1, 1, 161, T)).astype(np.float32)).to(dev)
    chunks = [spect[:, :, :, i:i + tc].contiguous() for i in range(0, T, tc)]
    for name, kind, H, L, bi in (("uni-LSTM-1024x5+lookahead", "lstm", 1024, 5, False), ("BiGRU-1024x5", "gru", 1024, 5, True)):
        cfg = dict(rnn_type=kind, hidden_size=H, hidden_layers=L, bidirectional=bi, lookahead_context=20)
        state = TP.random_state(cfg, 0)
        rt = getattr(configs.RNNType, kind)
        mc = configs.BiDirectionalConfig(rnn_type=rt, hidden_size=H, hidden_layers=L) if bi else \
            configs.UniDirectionalConfig(rnn_type=rt, hidden_size=H, hidden_layers=L, lookahead_context=20)
        for impl in (["ds2hip"] + (["stock-pytorch-rocm"] if a.stock else [])):
            if impl == "ds2hip":
                m = DeepSpeech(configs.LABELS, mc, "bf16", configs.AdamConfig(), configs.SpectConfig())
                m.load_state_dict({k: v.clone() for k, v in state.items()}, strict=True)
                m = m.to(dev).eval()

                def fn(c, hs, m=m):
                    with torch.no_grad():
                        out, _, hs2 = m(c, torch.tensor([c.shape[3]], dtype=torch.int), hs)
                    return out, hs2
            else:
                port = TP.Port(cfg, state, dev)

                def fn(c, hs, port=port):
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                        out, _, hs2 = port.forward(c, torch.tensor([c.shape[3]], dtype=torch.int), train=False, hs=hs, return_hs=True)
                    return out.float(), hs2
            if impl == "ds2hip" and a.carry:
                if bi:
                    continue                  # a reverse direction cannot be streamed exactly
                from deepspeech.pytorch_amd import decoder as D
                from deepspeech.pytorch_amd.streaming import StreamingTranscriber
                Ns = a.streams
                dec = D.BeamCTCDecoder(configs.LABELS, beam_width=a.beam_width) if a.decode == "beam" else D.GreedyDecoder(configs.LABELS)
                even = [c.expand(Ns, -1, -1, -1).contiguous() for c in chunks if c.shape[3] == tc]      # equal chunks only
                if a.wave:
                    spc = int(round(a.chunk * (a.rate or 16000)))
                    wav = torch.from_numpy(0.1 * rs.standard_normal((Ns, len(even) * spc)).astype(np.float32)).to(dev)
                    even = [wav[:, i * spc:(i + 1) * spc].contiguous() for i in range(len(even))]
                for carry in ((True,) if a.wave else (False, True)):
                    st = StreamingTranscriber(m, dec, front_end=_front_end(a), max_frames=T // 2 + len(chunks), carry_context=carry)
                    lat, total, text, emitted, frames = run_carry(st, even, a.reps, Ns, a.wave)
                    print(json.dumps({"metric": "session feed, chunked inference (StreamingTranscriber)", "model": name,
                                      "carry_context": carry, "input": "wave" if a.wave else "spectrogram",
                                      "input_rate": (a.rate or 16000) if a.wave else None, "decode": a.decode or "greedy",
                                      "streams": Ns, "audio_seconds": a.seconds,
                                      "chunk_seconds": a.chunk, "chunks": len(even), "latency_frames": st.latency_frames,
                                      "ms_per_feed_median": round(float(np.median(lat)) * 1e3, 3),
                                      "ms_per_feed_p95": round(float(np.percentile(lat, 95)) * 1e3, 3),
                                      "real_time_factor": round(a.seconds / total, 1), "out_frames_before_end": int(emitted),
                                      "out_frames": int(frames), "dtype": "bf16"}))
                continue
            if impl == "ds2hip" and a.decode:
                from deepspeech.pytorch_amd import decoder as D
                from deepspeech.pytorch_amd.streaming import StreamingTranscriber
                dec = D.GreedyDecoder(configs.LABELS) if a.decode == "greedy" else D.BeamCTCDecoder(configs.LABELS, beam_width=a.beam_width)
                lat, total, text, frames = run_decoding(StreamingTranscriber(m, dec, max_frames=T // 2 + len(chunks)), chunks, a.reps)
                print(json.dumps({"metric": "chunked batch-1 inference with streaming decode (StreamingTranscriber)", "model": name,
                                  "impl": impl, "decode": a.decode, "beam_width": a.beam_width if a.decode == "beam" else None,
                                  "audio_seconds": a.seconds, "chunk_seconds": a.chunk, "chunks": len(chunks),
                                  "ms_per_chunk_median": round(float(np.median(lat)) * 1e3, 3),
                                  "ms_per_chunk_p95": round(float(np.percentile(lat, 95)) * 1e3, 3),
                                  "real_time_factor": round(a.seconds / total, 1), "out_frames": int(frames[0]),
                                  "transcript_chars": len(text[0]), "dtype": "bf16"}))
                continue
            try:
                lat, total, out = run(fn, chunks, a.reps)
            except TypeError as e:            # the stock port has no hs plumbing: report and move on
                print(json.dumps({"model": name, "impl": impl, "error": str(e)[:200]}))
                continue
            print(json.dumps({"metric": "chunked batch-1 inference (reference inference.py:79-99)", "model": name, "impl": impl,
                              "audio_seconds": a.seconds, "chunk_seconds": a.chunk, "chunks": len(chunks),
                              "ms_per_chunk_median": round(float(np.median(lat)) * 1e3, 3),
                              "ms_per_chunk_p95": round(float(np.percentile(lat, 95)) * 1e3, 3),
                              "real_time_factor": round(a.seconds / total, 1), "out_frames": int(out.shape[1]), "dtype": "bf16"}))


if __name__ == "__main__":
    main()
    if "--carry" in sys.argv and "--wave" not in sys.argv:
        carry_error()
