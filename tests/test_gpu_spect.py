"""GPU parity of the spectrogram front-end (csrc/ds2_spect.hip) against the oracle's restatement of
SpectrogramParser.compute_spectrogram + _collate_fn (reference loader/data_loader.py:73-94, 247-270).

Behind the two original tests: the front-end at its length, tile, window and buffer edges.  Every comparison is against
O.log_spectrogram in fp64 with the one bound of the original test, max |device - oracle| < 2e-4, on normalised and on raw
log1p|X| outputs alike.  The waveforms live in tests/spect_cases.py, next to an fp32 numpy restatement of the pipeline (float32
DFT basis and matmul, fp32 log1p(sqrt), fp64 statistics, fp32 normalise); tests/test_spect_fp32_emulation.py holds that
restatement to 2e-5 of the oracle on every one of these cases, reflect padding and the one-frame clips included (its largest
figure is 1.3e-5), so the bound leaves the device at least 10x.  Every clip must be finite on the device except the one
all-zero clip whose reference is 0 / 0.  Largest error measured on an MI355X, per group of cases:
    frame-count edges (T and Tmax at 1, 2, 63..65, 127..129; both paddings, normalised and raw)   7.7e-6
    reflect padding of clips of 1..161 samples (raw)                                               3.3e-6
    hann / blackman / bartlett                                                                     3.3e-6
    signal classes (worst: noise on a 0.5 DC offset, normalised; raw 6.4e-6)                       1.44e-5
    a silent clip's neighbours                                                                     3.4e-6
    N = 65 and N = 1                                                                               2.7e-6
    480000 samples (3001 frames)                                                                   3.4e-6
    collate from int16-range samples                                                               2.8e-6
Overall maximum: 1.44e-5.  Each test prints its own figure (pytest -s).  The buffer-geometry, determinism and batch-independence
tests are bit-exact comparisons between device runs."""
import numpy as np
import pytest
import torch

import spect_cases as S
from oracle import ds2_oracle as O
from spect_cases import HOP, NBIN, noise, oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pad_mode,normalize", [("constant", True), ("reflect", True), ("constant", False)])
def test_spectrogram_batch_matches_oracle(pad_mode, normalize):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    rs = np.random.RandomState(7)
    lens = [24000, 23999, 16161, 8000, 801, 480]          # sorted descending like _collate_fn; odd lengths and a 3-frame clip
    wavs = [(rs.standard_normal(n) * rs.uniform(0.05, 0.6) + 0.01).astype(np.float32) for n in lens]
    fe = SpectrogramFrontEnd(configs.SpectConfig(), normalize=normalize, pad_mode=pad_mode)
    buf = torch.zeros((len(lens), max(lens)))
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = torch.from_numpy(w)
    inputs, pct, frames = fe(buf.cuda(), lens)
    Tmax = 1 + max(lens) // 160
    assert tuple(inputs.shape) == (len(lens), 1, 161, Tmax) and inputs.dtype == torch.float32
    got = inputs.cpu().numpy().astype(np.float64)
    for i, w in enumerate(wavs):
        ref = O.log_spectrogram(w.astype(np.float64), normalize=normalize, pad_mode=pad_mode)
        T = ref.shape[1]
        assert int(frames[i]) == T
        assert np.abs(got[i, 0, :, :T] - ref).max() < 2e-4, (i, np.abs(got[i, 0, :, :T] - ref).max())
        assert np.all(got[i, 0, :, T:] == 0)              # zero padding of the batch layout
        assert abs(float(pct[i]) - np.float32(T / float(Tmax))) < 1e-7
    # the percentages reproduce the frame counts through training_step's float round trip (model.py:243)
    assert (pct.cpu().mul(Tmax).int().numpy() == np.array([1 + n // 160 for n in lens])).all()


def test_spectrogram_feeds_the_model():
    """waveforms -> front-end -> training_step on the device: finite loss and gradients (the path of SURVEY 8(f)-3)."""
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.model import DeepSpeech
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    rs = np.random.RandomState(1)
    wavs = [rs.standard_normal(n).astype(np.float32) * 0.1 for n in (12000, 9000, 16000)]
    inputs, pct, order = SpectrogramFrontEnd(configs.SpectConfig()).collate(wavs)
    assert order == [2, 0, 1]
    torch.manual_seed(0)
    mc = configs.BiDirectionalConfig(rnn_type=configs.RNNType.gru, hidden_size=32, hidden_layers=2)
    m = DeepSpeech(configs.LABELS, mc, 32, configs.AdamConfig(), configs.SpectConfig()).cuda().train()
    targets = torch.from_numpy(rs.randint(1, 29, size=12).astype(np.int64))
    loss = m.training_step((inputs, targets, pct.clone(), torch.tensor([5, 4, 3], dtype=torch.int32)), 0)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())


# ---- length, tile, window and buffer edges ---------------------------------------------------------------------------------------
TOL = 2e-4                     # the bound of the test above, on normalised and on raw log1p|X| outputs alike
PATTERN = 0xA5                 # guard byte behind out / ws


def front_end(pad_mode="constant", normalize=True, window="hamming"):
    from deepspeech.pytorch_amd import configs
    from deepspeech.pytorch_amd.spectrogram import SpectrogramFrontEnd
    return SpectrogramFrontEnd(configs.SpectConfig(window=window), normalize=normalize, pad_mode=pad_mode)


def pack(wavs, width=None, fill=0.0):
    """[N][width] device buffer, row n = clip n followed by `fill`"""
    buf = np.full((len(wavs), width or max(len(w) for w in wavs)), fill, np.float32)
    for i, w in enumerate(wavs):
        buf[i, :len(w)] = w
    return torch.from_numpy(buf).cuda()


def check_batch(label, wavs, pad_mode="constant", normalize=True, window="hamming", nonfinite_ok=()):
    """One front-end call on `wavs` in the given order; frame counts, every clip against the fp64 oracle, exact zeros behind each
    clip, the percentages.  Every clip has to be finite on both sides and within TOL, except those the caller names in
    nonfinite_ok (indices of clips whose reference is 0 / 0 throughout; the caller judges their own frames).  Returns (largest
    |device - oracle| of the judged clips, the device output as fp64)."""
    lens = [len(w) for w in wavs]
    inputs, pct, frames = front_end(pad_mode, normalize, window)(pack(wavs), lens)
    Tmax = 1 + max(lens) // HOP
    assert tuple(inputs.shape) == (len(wavs), 1, NBIN, Tmax) and inputs.dtype == torch.float32
    got = inputs.cpu().numpy().astype(np.float64)
    errs = {}
    for i, w in enumerate(wavs):
        ref = oracle(w, pad_mode, normalize, window)
        T = 1 + lens[i] // HOP
        assert ref.shape == (NBIN, T) and int(frames[i]) == T
        assert np.all(got[i, 0, :, T:] == 0), (label, i)
        assert abs(float(pct[i]) - np.float32(T / float(Tmax))) < 1e-7
        if i in nonfinite_ok:
            assert not np.isfinite(ref).any(), (label, i)
            continue
        assert np.isfinite(ref).all(), (label, lens[i])
        assert np.isfinite(got[i, 0, :, :T]).all(), (label, lens[i])
        errs[i] = float(np.abs(got[i, 0, :, :T] - ref).max())
    assert (pct.mul(Tmax).int().numpy() == np.array([1 + n // HOP for n in lens])).all()
    worst = max(errs.values())
    per_clip = " ".join("%d:%.2e" % (lens[i], e) for i, e in errs.items()) if len(lens) <= 16 else "%d clips" % len(lens)
    print("%s [%s, %s, %s]: max |device - oracle| = %.3e  (%s)" % (label, pad_mode, "normalised" if normalize else "raw", window, worst, per_clip))
    for i, e in errs.items():
        assert e < TOL, (label, lens[i], e)
    return worst, got


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("batch", sorted(S.FRAME_BATCHES))
def test_frame_count_edges(batch, pad_mode, normalize):
    """A clip's own T on either side of the write kernel's 64-frame tile seams under a larger Tmax, and Tmax itself at 1, 2, 64,
    65 (a DFT GEMM of one or two overlapping rows).  The unnormalised runs carry a one-sample clip too: an impulse, whose
    spectrum is flat, so that it has no standard deviation to normalise by."""
    check_batch(batch, S.frame_edge_wavs(batch, normalize), pad_mode, normalize)


@pytest.mark.parametrize("L", S.REFLECT_LENGTHS)
def test_reflect_padding_of_short_clips_is_np_pad_reflect(L):
    """np.pad(mode="reflect") keeps folding a clip shorter than the 160-sample pad (period 2 (L - 1); one sample repeats), and so
    does the two-frame clip of 160 samples whose last frame reads padded index 319 = y[1].  Unnormalised, so that one wrong
    padded sample shows in the spectrum itself.  (A kernel that folds once and writes 0 for what is still outside the clip
    fails L = 1, 2, 41, 80 and 160 here and passes 81, 159, 161.)"""
    check_batch("reflect L=%d" % L, S.reflect_wavs(L), "reflect", False)


@pytest.mark.parametrize("window", S.WINDOWS)
def test_windows_reach_the_device(window):
    check_batch("window", S.window_wavs(), "constant", True, window)   # T = 65, 64, 3


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", S.SIGNAL_KINDS)
def test_signal_classes(kind, normalize):
    check_batch(kind, S.signal_wavs(kind), "constant", normalize)


@pytest.mark.parametrize("normalize", [True, False])
def test_silent_clip_between_two_ordinary_ones(normalize):
    """An all-zero clip has mean 0 and std 0: normalised it is 0 / 0 in the reference (NaN over its own frames), and the device
    must not let that leak into its padding frames or its neighbours; unnormalised it is exactly 0."""
    wavs = S.silent_wavs()
    # neighbours within tolerance, padding frames zero, frame counts; normalised, clip 1 is the one 0 / 0 reference of this file
    _, got = check_batch("silent", wavs, "constant", normalize, nonfinite_ok={1} if normalize else ())
    T = 1 + len(wavs[1]) // HOP
    if normalize:
        assert not np.isfinite(got[1, 0, :, :T]).any()            # exactly where the oracle is non-finite: all of its own frames
    else:
        assert np.all(got[1, 0] == 0)


def raw_spectrogram(fe, wav, lens, extra=0):
    """ds2_spectrogram through the raw ABI on byte buffers that are `extra` bytes longer than needed and pre-filled with PATTERN.
    Returns (out (N, 1, 161, Tmax) as a view of its buffer, the out buffer, the ws buffer, bytes needed of out, of ws)."""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    N, Lm = len(lens), max(lens)
    Tmax = 1 + Lm // HOP
    need_out, need_ws = N * NBIN * Tmax * 4, query("ds2_spect_ws_bytes", N, Lm)
    out = torch.full((need_out + extra,), PATTERN, dtype=torch.uint8, device=wav.device)
    ws = torch.full((need_ws + extra,), PATTERN, dtype=torch.uint8, device=wav.device)
    ns = torch.tensor(lens, dtype=torch.int32, device=wav.device)
    assert wav.stride(1) == 1 and wav.stride(0) >= Lm
    call("ds2_spectrogram", ops.P(wav), wav.stride(0), ops.P(ns), N, Lm, ops.P(fe._basis_on(wav.device)), 1 if fe.reflect else 0,
         1 if fe.normalize else 0, ops.P(out), ops.P(ws), ops.S())
    torch.cuda.synchronize()
    return out[:need_out].view(torch.float32).view(N, 1, NBIN, Tmax), out, ws, need_out, need_ws


GEOMETRY = {1: [801], 3: [10240, 801, 159]}


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("N", [1, 3])
def test_row_stride_and_samples_behind_a_clip_are_not_read(N, pad_mode):
    """ldw = Lmax + 37 and 1e3 in every sample at or behind nsamples[n]: bit for bit the output of the tight, zero-filled buffer."""
    lens = GEOMETRY[N]
    wavs = [noise(500 + k, n) for k, n in enumerate(lens)]
    fe = front_end(pad_mode)
    tight = raw_spectrogram(fe, pack(wavs), lens)[0]
    wide = raw_spectrogram(fe, pack(wavs, max(lens) + 37, 1e3), lens)[0]
    assert torch.isfinite(tight).all() and torch.equal(tight, wide)


@pytest.mark.parametrize("Lmax", [159, 801, 10240])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_kernels_stay_inside_out_and_the_workspace(N, Lmax):
    """N * 161 * Tmax * 4 bytes of out and ds2_spect_ws_bytes(N, Lmax) of ws are all the call may touch (an odd N moves the
    16-byte round-up in front of the fp64 partial sums): 4096 patterned bytes behind each are as they were."""
    lens = [Lmax, max(1, Lmax // 2), 2][:N]
    wavs = [noise(600 + k, n) for k, n in enumerate(lens)]
    fe = front_end("reflect")
    wav = pack(wavs)
    ref, _, _ = fe(wav, lens)                                         # the production entry: the raw helper makes the same call
    got, out, ws, need_out, need_ws = raw_spectrogram(fe, wav, lens, extra=4096)
    assert torch.equal(got, ref) and torch.isfinite(ref).all()
    assert out.numel() == need_out + 4096 and bool((out[need_out:] == PATTERN).all())
    assert ws.numel() == need_ws + 4096 and bool((ws[need_ws:] == PATTERN).all())


def test_front_end_takes_a_buffer_wider_than_the_longest_clip():
    lens = GEOMETRY[3]
    wavs = [noise(500 + k, n) for k, n in enumerate(lens)]
    fe = front_end()
    a, pa, fa = fe(pack(wavs), lens)
    b, pb, fb = fe(pack(wavs, max(lens) + 37, 1e3), lens)
    assert a.shape == b.shape and torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(fa, fb)


def test_batch_of_65_crosses_the_finalize_block():
    """k_spect_finalize runs 64 clips per block: 65 clips of 2 to 4 frames, all of different lengths, each against the oracle."""
    check_batch("N=65", S.n65_wavs())


def test_batch_of_one():
    check_batch("N=1", S.n1_wavs())


def test_deterministic_and_independent_of_the_rest_of_the_batch():
    """The K order of the DFT GEMM is the same for every output element and k_spect_stats strides over a clip's own frames by a
    fixed block count, so neither Tmax nor N reaches a clip's values: the same call twice, and a clip alone against its rows in a
    batch beside longer clips, agree bit for bit."""
    lens = [20480, 10240, 10239, 480, 159]
    wavs = [noise(900 + k, n) for k, n in enumerate(lens)]
    fe = front_end()
    wav = pack(wavs)
    a, _, _ = fe(wav, lens)
    b, _, _ = fe(wav, lens)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    for i, w in enumerate(wavs):
        alone, _, _ = fe(pack([w]), [lens[i]])
        T = 1 + lens[i] // HOP
        assert tuple(alone.shape) == (1, 1, NBIN, T)
        assert torch.equal(alone[0], a[i, :, :, :T]), (lens[i], float((alone[0] - a[i, :, :, :T]).abs().max()))


def test_long_clip():
    """30 s: 3001 frames through the long index arithmetic and ~94 frames per block of the strided statistics loop."""
    check_batch("L=480000", S.long_wavs())


def test_collate_with_transcripts_and_int16_scale():
    """_collate_fn's whole batch tuple from int16-range samples given out of length order, one transcript empty."""
    rs = np.random.RandomState(12)
    lens = [801, 10240, 480]
    waves = [torch.from_numpy(np.round(3000.0 * rs.standard_normal(n)).clip(-32767, 32767).astype(np.float32)) for n in lens]
    transcripts = [[3, 1, 4, 1, 5], [], [9, 2, 6]]
    inputs, targets, pct, target_sizes = front_end().collate(waves, transcripts=transcripts, int16_scale=True)
    order = [1, 0, 2]
    Tmax = 1 + max(lens) // HOP
    assert tuple(inputs.shape) == (3, 1, NBIN, Tmax)
    got = inputs.cpu().numpy().astype(np.float64)
    worst = 0.0
    for r, i in enumerate(order):
        ref = oracle(waves[i].numpy().astype(np.float64) / 32767.0, "constant", True)
        T = ref.shape[1]
        worst = max(worst, float(np.abs(got[r, 0, :, :T] - ref).max()))
        assert np.all(got[r, 0, :, T:] == 0)
        assert abs(float(pct[r]) - np.float32(T / float(Tmax))) < 1e-7
    print("collate: max |device - oracle| = %.3e" % worst)
    assert worst < TOL
    assert targets.dtype == torch.int64 and targets.tolist() == [3, 1, 4, 1, 5, 9, 2, 6]
    assert target_sizes.dtype == torch.int32 and target_sizes.tolist() == [0, 5, 3]
