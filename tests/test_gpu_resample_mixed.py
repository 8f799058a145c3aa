"""GPU checks of per-clip sample rates ("Mixed rates"; csrc/ds2_resample.hip: k_resample_mixed,
k_resample_stream_mixed, k_resample_stream_carry_mixed; resample.ResamplerBank / BankStream, SpectrogramFrontEnd(input_rate=(...)),
StreamPool.open(rate=...), WaveAugment(speed_choices=...), NoiseBank.from_waveforms(rates=...)).

Everything here is torch.equal.  With integer taps and integer samples every sum stays below 2^24 (|h| <= 8, |x| <= 64, at most
9600 taps), so the device must give the integers of the definition restated in numpy (tests/resample_reference.py).  With the real
taps a row of a mixed launch must be the row of the single-rate launch of its class, and a streamed row the one-shot row: the order
of a sample's sum depends on the tap index alone."""
import ctypes

import numpy as np
import pytest
import torch

import resample_reference as RR
from fixtures import DEV, Fixture
from test_gpu_model import build
from test_gpu_resample import GARBAGE, UNSTAGED, clip, front_end, inputs_for, pack, run_streams

pytestmark = pytest.mark.gpu
HOP = 160
COPY = (1, 1, 0)
#          8000         48000       44100           14400 (16 kHz x 0.9)  17600 (x 1.1)
CLASSES = [(2, 1, 24), (1, 3, 72), (160, 441, 67), (10, 9, 24), (10, 11, 27), COPY, UNSTAGED]
WORDS = 10                                                                  # int32 words of one ds2_resample_class


def class_table(udw):
    """ds2_resample_classes -> (the host table as int32 [C * 10], tiles [C], taps_off [C], floats of the taps buffer)"""
    from deepspeech.pytorch_amd._lib import call
    udw = np.ascontiguousarray(udw, dtype=np.int32)
    table, total = np.zeros(len(udw) * WORDS, np.int32), ctypes.c_long(-1)
    call("ds2_resample_classes", ctypes.c_void_p(udw.ctypes.data), len(udw), ctypes.c_void_p(table.ctypes.data), ctypes.byref(total))
    t = table.reshape(-1, WORDS)
    return table, t[:, 6].tolist(), t[:, 8:10].copy().view(np.int64).reshape(-1).tolist(), total.value


def integer_bank(udw):
    """(host table, device table, device taps, per-class integer tables, tiles) with RR.integer_taps as every class's table"""
    table, tiles, offs, total = class_table(udw)
    hs = [RR.integer_taps(U, W) if W else None for U, D, W in udw]
    taps = np.zeros(total, np.float32)
    for h, o in zip(hs, offs):
        if h is not None:
            taps[o:o + h.size] = h.reshape(-1)
    return table, torch.from_numpy(table).to(DEV), torch.from_numpy(taps).to(DEV), hs, tiles


def reference(x, h, U, D, W):
    return np.asarray(x) if W == 0 else RR.resample(x, h, U, D, W)


def out_len(n, U, D, W):
    return int(n) if W == 0 else RR.out_len(n, U, D)


def mixed(clips, cls, bank, ldo=None, pad=13):
    """ops.resample_mixed on a garbage-padded buffer -> (out, nsamples_out)"""
    from deepspeech.pytorch_amd import ops
    table, table_dev, taps = bank[:3]
    lens = [len(c) for c in clips]
    buf = torch.full((len(clips), max(lens) + pad), GARBAGE)
    for i, c in enumerate(clips):
        buf[i, :len(c)] = torch.from_numpy(np.asarray(c, dtype=np.float32))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                      # noqa: E731
    return ops.resample_mixed(buf.to(DEV), i32(lens), i32(cls), table, table_dev, taps, ldo)


# ---- 1. integer operands, bit for bit ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_bank():
    return integer_bank(CLASSES)


def test_the_class_table_is_rs_cfg_per_class_and_the_tables_lie_back_to_back():
    from deepspeech.pytorch_amd._lib import query
    table, tiles, offs, total = class_table(CLASSES)
    want_off = 0
    for (U, D, W), tile, off in zip(CLASSES, tiles, offs):
        assert off == want_off and off % 2 == 0
        if W:
            assert tile == query("ds2_resample_tile", U, D, W)
        want_off += U * 2 * W
    assert total == want_off and tiles[CLASSES.index(COPY)] == 4096
    assert table.reshape(-1, WORDS)[CLASSES.index(UNSTAGED), 7] == 0                    # no staged span: the other body


@pytest.mark.parametrize("first", range(len(CLASSES)))
def test_integer_operands_of_seven_classes_in_one_launch_equal_the_oracle(int_bank, first):
    """seven launches of seven rows, one per class: launch r starts with class r and ends with class r - 1, neighbours differ in
    class, and over the launches every class gets clips of 1 output and of tile - 1, tile and tile + 1 outputs (where U > D only
    every other count exists: the nearest above)"""
    hs, tiles = int_bank[3:]
    C = len(CLASSES)
    kind_of = lambda r, i: (r + 2 * i) % 4                                              # noqa: E731
    for c in range(C):                                                                  # the schedule covers every kind per class
        assert {kind_of(r, (c - r) % C) for r in range(C)} == {0, 1, 2, 3}
    rng = np.random.RandomState(first)
    cls = [(first + i) % C for i in range(C)]
    clips = []
    for i, c in enumerate(cls):
        U, D, W = CLASSES[c]
        outputs = (1, tiles[c] - 1, tiles[c], tiles[c] + 1)[kind_of(first, i)]
        n = outputs if W == 0 else max(1, inputs_for(outputs, U, D))
        clips.append(rng.randint(-64, 65, size=n).astype(np.int64))
    lens16 = [out_len(len(x), *CLASSES[c]) for x, c in zip(clips, cls)]
    out, ns_out = mixed(clips, cls, int_bank, max(lens16))
    assert ns_out.tolist() == lens16
    for i, (x, c) in enumerate(zip(clips, cls)):
        want = reference(x, hs[c], *CLASSES[c])
        assert len(want) == lens16[i] and np.abs(want).max() < 2 ** 24
        assert torch.equal(out[i, :len(want)].cpu(), torch.from_numpy(want.astype(np.float32))), (first, i, CLASSES[c])
        assert not out[i, len(want):].any()


def test_the_copy_class_keeps_the_bits_and_an_unknown_class_gives_zeros(int_bank):
    """-0.0, a denormal, inf and nan pass the copy class as they are; rows of class -1 and C are zeros with a count of 0 and
    leave their neighbours alone"""
    x = np.array([-0.0, 1e-42, np.inf, np.nan, -3.5, 0.0], np.float32)
    y = np.arange(1, 50, dtype=np.float32)
    cp = CLASSES.index(COPY)
    out, ns_out = mixed([x, y, x, y, y], [cp, -1, cp, len(CLASSES), 0], int_bank, 98)
    assert ns_out.tolist() == [6, 0, 6, 0, 98]
    for r in (0, 2):
        assert torch.equal(out[r, :6].cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32)) and not out[r, 6:].any()
    assert not out[1].any() and not out[3].any()
    want = RR.resample(y.astype(np.int64), int_bank[3][0], *CLASSES[0])
    assert torch.equal(out[4].cpu(), torch.from_numpy(want.astype(np.float32)))


# ---- 2. real taps against the single-rate path -----------------------------------------------------------------------------------
RATES = (8000, 16000, 48000, 44100, 11025, 14400, 17600)


@pytest.fixture(scope="module")
def real_bank():
    from deepspeech.pytorch_amd.resample import ResamplerBank
    return ResamplerBank(RATES)


def test_every_row_of_a_mixed_call_equals_the_single_rate_call_on_that_clip(real_bank):
    from deepspeech.pytorch_amd.resample import Resampler
    rates = [48000, 8000, 16000, 44100, 11025, 8000, 17600, 14400, 48000, 16000, 44100]
    lens = [3001, 1500, 2000, 2756, 700, 1, 1100, 2999, 72, 1, 4410]
    wavs = [clip(200 + k, n) for k, n in enumerate(lens)]
    out, ns16 = real_bank(pack(wavs, max(lens) + 5), lens, rates)
    assert ns16.tolist() == [real_bank.out_len(n, r) for n, r in zip(lens, rates)] and out.shape[1] == max(ns16.tolist())
    for i, (w, r) in enumerate(zip(wavs, rates)):
        rs = Resampler(r)
        assert np.array_equal(rs.taps, real_bank.resampler(r).taps)
        want, n16 = rs(pack([w]), [len(w)])
        assert int(n16[0]) == int(ns16[i])
        assert torch.equal(out[i, :int(n16[0])], want[0, :int(n16[0])]) and not out[i, int(n16[0]):].any(), (i, r)


# ---- 3. streaming == one-shot, bit for bit ---------------------------------------------------------------------------------------
STREAM_RATES = [8000, 48000, 44100, 16000]


def width(rate):
    return RR.params(rate)[2] if rate != 16000 else 24


_ONE_SHOT = {}


def one_shot(bank, rates, lens, seed):
    key = (tuple(rates), tuple(lens), seed)
    if key not in _ONE_SHOT:
        wavs = [clip(seed + 7 * k + n, n) for k, n in enumerate(lens)]
        out, ns16 = bank(pack(wavs), lens, rates)
        _ONE_SHOT[key] = (wavs, out.clone(), ns16.tolist())
    return _ONE_SHOT[key]


@pytest.mark.parametrize("feed", ["1", "W-1", "W", "W+1", "2W", "97", "whole"])
def test_slots_at_different_rates_fed_in_one_call_equal_the_one_shot_rows(real_bank, feed):
    """four clips of 6W + 5 samples (W that of the row's class; the copy class: 24) at 8000, 48000, 44100 and 16000 Hz on slots 3,
    0, 2, 1 of five; a row brings its own W-sized chunk a tick, empty feeds in between"""
    Ws = [width(r) for r in STREAM_RATES]
    lens = [6 * W + 5 for W in Ws]
    wavs, ref, ns16 = one_shot(real_bank, STREAM_RATES, lens, 100)
    per_row = [{"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "2W": 2 * W, "97": 97, "whole": None}[feed] for W in Ws]
    st = real_bank.stream(5, DEV)
    with pytest.raises(ValueError, match="no rate"):
        st.feed([3], pack([wavs[0][:4]]), [4])
    st.reset([3, 0, 2, 1], STREAM_RATES)
    got = run_streams(st, [3, 0, 2, 1], wavs, per_row, seed=len(feed) + (per_row[0] or 0))
    for r, n16 in enumerate(ns16):
        assert got[r].shape[0] == n16 and torch.equal(got[r], ref[r, :n16]), (feed, r)
    assert st.samples == [lens[1], lens[3], lens[2], lens[0], 0] and st.ended == [True] * 4 + [False]


def test_a_final_feed_of_nothing_flushes_the_tails_of_every_class(real_bank):
    lens = [1000, 4410, 3000, 500]
    wavs, ref, ns16 = one_shot(real_bank, STREAM_RATES, lens, 500)
    st = real_bank.stream(4, DEV)
    st.reset(None, STREAM_RATES)
    a, e = st.feed([0, 1, 2, 3], pack(wavs), lens)
    b, f = st.feed([3, 2, 1, 0], torch.zeros((4, 0), device=DEV), [0] * 4, final=[0, 1, 2, 3])
    assert [e[r] + f[3 - r] for r in range(4)] == ns16 and min(f[1:]) > 0 and f[0] == 0     # the copy class has no tail
    for r in range(4):
        assert torch.equal(torch.cat([a[r, :e[r]], b[3 - r, :f[3 - r]]]), ref[r, :ns16[r]])


@pytest.mark.parametrize("rates", [(8000, 48000), (48000, 8000)])
def test_a_slot_reused_at_another_rate_starts_fresh_and_the_others_keep_their_state(real_bank, rates):
    """slot 1 is left in the middle of a loud stream at rates[0] (W 24 <-> 72) and reused at rates[1] while slots 0 and 3 run"""
    old, new = rates
    Wn = width(new)
    lens = [6 * Wn + 5]
    wavs, ref, ns16 = one_shot(real_bank, [new], lens, 300)
    st = real_bank.stream(4, DEV)
    Wmax = real_bank.half_width
    loud = clip(1, 400, 0.7) + 0.3
    st.reset([0, 1, 3], [44100, old, 48000])
    st.feed([0, 1, 3], pack([loud, loud, loud]), [300, 400, 350])
    state = lambda: st._state.view(torch.float32).view(4, 2 * Wmax).clone()                # noqa: E731
    before = state()
    assert before[[0, 1, 3]].any(1).all() and not before[2].any()
    st.reset([1], [new])
    assert torch.equal(state(), before)                                                   # reset launches nothing
    got = []
    a, e = st.feed([1], pack([wavs[0][:7]]), [7])
    got.append(a[0, :e[0]])
    after = state()
    assert torch.equal(after[[0, 2, 3]], before[[0, 2, 3]])
    assert torch.equal(after[1, :7].cpu(), torch.from_numpy(wavs[0][:7]))
    a, e = st.feed([3, 1], pack([loud[:40], wavs[0][7:7 + 2 * Wn]], 2 * Wn), [40, 2 * Wn])  # slot 3 goes on beside it
    got.append(a[1, :e[1]])
    assert torch.equal(state()[[0, 2]], before[[0, 2]])
    a, e = st.feed([1], pack([wavs[0][7 + 2 * Wn:]]), [lens[0] - 7 - 2 * Wn], final=[1])
    got.append(a[0, :e[0]])
    assert torch.equal(torch.cat(got), ref[0, :ns16[0]])
    # slots 0 and 3 were not disturbed: their streams end as the one-shot rows of what they were fed
    tail, f = st.feed([0, 3], torch.zeros((2, 0), device=DEV), [0, 0], final=[0, 3])
    want, n16 = real_bank(pack([loud[:300], np.concatenate([loud[:350], loud[:40]])]), [300, 390], [44100, 48000])
    for r, row in enumerate(tail):
        assert torch.equal(row[:f[r]], want[r, int(n16[r]) - f[r]:int(n16[r])])


# ---- 4. writes stay inside -------------------------------------------------------------------------------------------------------
def test_the_kernels_write_nothing_outside_out_the_workspace_and_the_state(real_bank):
    """through the raw ABI on buffers 1024 patterned floats longer than needed: a batch of the narrowest class (the copy class,
    W = 0), 8000 Hz (W = 24) and the widest of the bank (48000 Hz, W = 72); one-shot, then two feeds (the second final)"""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    rates, lens = [16000, 48000, 8000], [700, 2101, 333]
    cls = [real_bank.class_of[r] for r in rates]
    wavs = [clip(900 + k, n) for k, n in enumerate(lens)]
    wav = pack(wavs)
    table_dev, taps = real_bank.on(wav.device)
    host = ctypes.c_void_p(real_bank.classes.ctypes.data)
    C, Wmax = len(RATES), real_bank.half_width
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                      # noqa: E731
    want, ns16 = real_bank(wav, lens, rates)
    ldo = want.shape[1]
    out = torch.full((3 * ldo + 1024,), GARBAGE, device=DEV)
    ns_out = torch.full((3 + 64,), -7, dtype=torch.int32, device=DEV)
    ns_dev, cls_dev = i32(lens), i32(cls)
    call("ds2_resample_mixed", ops.P(wav), wav.stride(0), ops.P(ns_dev), ops.P(cls_dev), 3, host, ops.P(table_dev), C, ops.P(taps),
         ops.P(out), ldo, ops.P(ns_out), ops.S())
    torch.cuda.synchronize()
    assert torch.equal(out[:3 * ldo].view(3, ldo), want) and bool((out[3 * ldo:] == GARBAGE).all())
    assert ns_out[:3].tolist() == ns16.tolist() and bool((ns_out[3:] == -7).all())
    # streamed: slots 1, 2, 3 of four
    S = 4
    need_state = query("ds2_resample_stream_state_bytes_mixed", S, Wmax) // 4
    assert need_state == S * 2 * Wmax
    state = torch.full((need_state + 1024,), GARBAGE, device=DEV)
    handle = real_bank.stream(S, DEV)
    handle.reset([1, 2, 3], rates)
    done = [0, 0, 0]
    for final in (False, True):
        cnt = [n - d for n, d in zip(lens, done)] if final else [n // 2 for n in lens]
        chunk = pack([w[d:d + c] for w, d, c in zip(wavs, done, cnt)])
        plans = [real_bank.plan_resample(r, d, c, final) for r, d, c in zip(rates, done, cnt)]
        me, mx = max(p.emit for p in plans), max(cnt)
        table = np.zeros((3, 10), np.int32)
        for r, (c, p, k) in enumerate(zip(cnt, plans, cls)):
            copy = rates[r] == 16000
            table[r, :4] = (r + 1, r, 0 if copy else p.carried, c)
            table[r, 4:6] = np.array([0 if copy else p.out_before], np.int64).view(np.int32)
            table[r, 6:] = (p.emit, int(final), int(not final), k)
        table = torch.from_numpy(table).to(DEV)
        need_ws = query("ds2_resample_stream_ws_bytes_mixed", 3, Wmax) // 4
        out = torch.full((3 * me + 1024,), GARBAGE, device=DEV)
        ws = torch.full((need_ws + 1024,), GARBAGE, device=DEV)
        call("ds2_resample_stream_feed_mixed", ops.P(chunk), chunk.stride(0), ops.P(table), 3, mx, me, S, host, ops.P(table_dev), C,
             ops.P(taps), Wmax, ops.P(state), ops.P(out), me, ops.P(ws), ops.S())
        torch.cuda.synchronize()
        ref, emitted = handle.feed([1, 2, 3], chunk, cnt, final=[1, 2, 3] if final else ())
        assert emitted == [p.emit for p in plans]
        assert torch.equal(out[:3 * me].view(3, me), ref)
        assert bool((out[3 * me:] == GARBAGE).all()) and bool((ws[need_ws:] == GARBAGE).all())
        assert bool((state[need_state:] == GARBAGE).all()) and bool((state[:2 * Wmax] == GARBAGE).all())   # slot 0 is in no row
        assert bool((state[2 * Wmax:4 * Wmax] == GARBAGE).all())                         # the copy class keeps nothing in its slot
        for slot, r in ((2, 48000), (3, 8000)):                                          # a slot keeps at most 2 W_c - 1 samples
            W = RR.params(r)[2]
            assert bool((state[slot * 2 * Wmax + 2 * W - 1:(slot + 1) * 2 * Wmax] == GARBAGE).all())
        done = [d + c for d, c in zip(done, cnt)]


# ---- 5. a row table given directly, out_before beyond 2^31 -----------------------------------------------------------------------
def test_rows_with_out_before_beyond_2_to_the_31(int_bank):
    """two streams far into their utterances, 44100 Hz and 8000 Hz, through the raw ABI: the carry and the new samples are given,
    the outputs are the oracle's for those positions"""
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import call, query
    host, table_dev, taps, hs, _ = int_bank
    Wmax = max(W for _, _, W in CLASSES)
    S, n_new = 3, 1500
    rng = np.random.RandomState(31)
    state = torch.zeros(query("ds2_resample_stream_state_bytes_mixed", S, Wmax) // 4, device=DEV)
    table, chunks, want = np.zeros((2, 10), np.int32), [], []
    for r, (c, G0) in enumerate(((2, 6_000_000_123), (0, (1 << 30) + 4567))):
        U, D, W = CLASSES[c]
        e0, emit, carried, new_carry, f0 = RR.plan(G0, n_new, False, U, D, W)
        assert e0 > 2 ** 31 and emit > 0 and 0 < carried < 2 * W
        x = rng.randint(-64, 65, size=carried + n_new).astype(np.int64)                 # clip positions [f0, G0 + n_new)
        state.view(S, 2 * Wmax)[r + 1, :carried] = torch.from_numpy(x[:carried].astype(np.float32)).to(DEV)
        chunks.append(x[carried:].astype(np.float32))
        want.append(RR.resample(x, hs[c], U, D, W, ms=np.arange(e0, e0 + emit, dtype=np.int64), first=f0, end=G0 + n_new))
        table[r, :4] = (r + 1, r, carried, n_new)
        table[r, 4:6] = np.array([e0], np.int64).view(np.int32)
        table[r, 6:] = (emit, 0, 0, c)
    me = max(len(w) for w in want)
    chunk, rows = pack(chunks), torch.from_numpy(table).to(DEV)
    out = torch.full((2, me), GARBAGE, device=DEV)
    ws = torch.empty(query("ds2_resample_stream_ws_bytes_mixed", 2, Wmax) // 4, device=DEV)
    call("ds2_resample_stream_feed_mixed", ops.P(chunk), chunk.stride(0), ops.P(rows), 2, n_new, me, S, ctypes.c_void_p(host.ctypes.data),
         ops.P(table_dev), len(CLASSES), ops.P(taps), Wmax, ops.P(state), ops.P(out), me, ops.P(ws), ops.S())
    for r, w in enumerate(want):
        assert torch.equal(out[r, :len(w)].cpu(), torch.from_numpy(w.astype(np.float32))) and not out[r, len(w):].any()


# ---- 6. the front-end ------------------------------------------------------------------------------------------------------------
FE_RATES = (8000, 16000, 48000, 44100)


@pytest.mark.parametrize("normalize", [True, False, "running"])
def test_front_end_with_a_set_of_rates_equals_the_single_rate_front_end_per_clip(normalize):
    rates, lens = [44100, 8000, 16000, 48000, 8000], [9000, 4410, 3000, 300, 161]
    wavs = [clip(40 + k, n) for k, n in enumerate(lens)]
    fe = front_end(normalize, input_rate=FE_RATES)
    got, pct, frames = fe(pack(wavs, 9100), lens, rates=rates)
    for i, (w, r) in enumerate(zip(wavs, rates)):
        want, _, fr = front_end(normalize, input_rate=r)(pack([w]), [len(w)])
        assert int(fr[0]) == int(frames[i]) == 1 + fe.bank.out_len(len(w), r) // HOP
        assert torch.equal(got[i, :, :, :int(fr[0])], want[0]), (normalize, i)
    assert got.shape[3] == int(frames.max())
    assert pct.tolist() == [np.float32(f / float(frames.max())) for f in frames.tolist()]
    with pytest.raises(ValueError, match="rates"):
        fe(pack(wavs), lens)
    with pytest.raises(ValueError, match="rates"):
        fe(pack(wavs), lens, rates=[22050] * 5)
    with pytest.raises(ValueError, match="single input rate"):
        front_end(normalize, input_rate=8000)(pack(wavs), lens, rates=rates)
    # collate sorts by the 16 kHz lengths and is the call on the sorted batch
    inputs, cpct, order = fe.collate([torch.from_numpy(w) for w in wavs], rates=rates)
    assert order == sorted(range(5), key=lambda i: -fe.bank.out_len(lens[i], rates[i]))
    want, wpct, _ = fe(pack([wavs[i] for i in order]), [lens[i] for i in order], rates=[rates[i] for i in order])
    assert torch.equal(inputs, want) and torch.equal(cpct, wpct)


def test_front_end_stream_at_mixed_rates_equals_the_one_shot_running_call():
    """chunks of 441, 4410 and 1000 samples in turn on slots at 44100, 8000 and 16000 Hz"""
    rates, lens = [44100, 8000, 16000], [30000, 9000, 12345]
    wavs = [clip(70 + k, n) for k, n in enumerate(lens)]
    fe = front_end(input_rate=FE_RATES)
    ref, _, frames = fe(pack(wavs), lens, rates=rates)
    st = fe.stream(4, DEV)
    slots, pos, got, k, live = [2, 0, 3], [0, 0, 0], [[], [], []], 0, [0, 1, 2]
    with pytest.raises(ValueError, match="no rate"):
        st.feed([2], pack([wavs[0][:10]]), [10])
    st.reset(slots, rates=rates)
    while live:
        c = (441, 4410, 1000)[k % 3]
        counts = [min(c, lens[r] - pos[r]) for r in live]
        final = [r for r, n in zip(live, counts) if pos[r] + n == lens[r]]
        out, fr = st.feed([slots[r] for r in live], pack([wavs[r][pos[r]:pos[r] + n] for r, n in zip(live, counts)]), counts,
                          final=[slots[r] for r in final])
        for i, r in enumerate(live):
            got[r].append(out[i, 0, :, :fr[i]])
            pos[r] += counts[i]
        live, k = [r for r in live if r not in final], k + 1
    for r in range(3):
        assert st.frames(slots[r]) == frames[r] and st.samples[slots[r]] == fe.bank.out_len(lens[r], rates[r])
        assert torch.equal(torch.cat(got[r], 1), ref[r, 0, :, :frames[r]])
    with pytest.raises(ValueError, match="set of rates"):
        front_end(input_rate=8000).stream(2, DEV).reset([0], rates=[8000])


# ---- 7. the pool -----------------------------------------------------------------------------------------------------------------
def test_pool_with_slots_at_three_rates_equals_the_pool_fed_the_resampled_audio():
    """streams at 8000, 16000 and 44100 Hz that join one tick apart, 0.1 s of audio a tick each.  The reference pool gets the
    one-shot-resampled clips in the chunks the plan says each feed emits: the same transcripts after every feed and the same
    probabilities, torch.equal"""
    from deepspeech.pytorch_amd import decoder as Dc
    from deepspeech.pytorch_amd.streaming import StreamPool
    fx = Fixture("gru_uni_la")
    m = build(fx, 32).eval()
    rates, lens = [8000, 16000, 44100], [6000, 11000, 30000]
    rng = np.random.RandomState(17)
    wavs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    fe = front_end(input_rate=(8000, 16000, 44100))
    out, ns16 = fe.bank(pack(wavs), lens, rates)
    wavs16 = [out[i, :n].cpu().numpy() for i, n in enumerate(ns16.tolist())]
    dec = Dc.GreedyDecoder(fx.labels)
    pool, ref = StreamPool(m, dec, 3, front_end=fe), StreamPool(m, dec, 3, front_end=front_end())
    with pytest.raises(ValueError, match="open\\(rate"):
        pool.open()
    with pytest.raises(ValueError, match="open\\(rate"):
        pool.open(rate=22050)
    with pytest.raises(ValueError, match="one input rate"):
        ref.open(rate=8000)
    slot, pos, pos16, got, want, done, tick = {}, {}, {}, {r: [] for r in range(3)}, {r: [] for r in range(3)}, set(), 0
    while len(done) < 3:
        if tick < 3:
            slot[tick] = pool.open(rate=rates[tick])
            assert ref.open() == slot[tick]
            pos[tick] = pos16[tick] = 0
        rows = [r for r in slot if r not in done]
        counts = [min(rates[r] // 10, lens[r] - pos[r]) for r in rows]
        final = [r for r, c in zip(rows, counts) if pos[r] + c == lens[r]]
        plans = [fe.bank.plan_resample(rates[r], pos[r], c, r in final) for r, c in zip(rows, counts)]
        assert all(p.out_before == pos16[r] for r, p in zip(rows, plans))
        t1 = pool.feed_wave([slot[r] for r in rows], pack([wavs[r][pos[r]:pos[r] + c] for r, c in zip(rows, counts)]), counts,
                            final=[slot[r] for r in final])
        t2 = ref.feed_wave([slot[r] for r in rows], pack([wavs16[r][pos16[r]:pos16[r] + p.emit] for r, p in zip(rows, plans)]),
                           [p.emit for p in plans], final=[slot[r] for r in final])
        assert t1 == t2, tick
        assert set(pool.last_output) == set(ref.last_output)
        for r, c, p in zip(rows, counts, plans):
            if slot[r] in pool.last_output:
                got[r].append(pool.last_output[slot[r]])
                want[r].append(ref.last_output[slot[r]])
            pos[r], pos16[r] = pos[r] + c, pos16[r] + p.emit
        done |= set(final)
        tick += 1
    for r in range(3):
        assert pos16[r] == len(wavs16[r]) and torch.cat(got[r]).shape[0] > 0
        assert torch.equal(torch.cat(got[r]), torch.cat(want[r]))


# ---- 8. speed perturbation -------------------------------------------------------------------------------------------------------
def test_speed_perturbation_equals_the_resampler_at_rate_times_speed_then_the_remaining_draws():
    """the draws of a seeded rng are replayed on the host (WaveAugment.draw with the same seed): every clip must come out as
    Resampler(rate * speed) on that clip, followed by the 16 kHz front-end handed the same tempo / gain draws"""
    from deepspeech.pytorch_amd.augment import WaveAugment, speed_rate
    from deepspeech.pytorch_amd.resample import Resampler
    rates, lens = [48000, 16000, 8000, 16000, 48000, 8000], [9000, 4000, 2500, 3100, 6000, 1800]
    wavs = [clip(80 + k, n) for k, n in enumerate(lens)]
    wa = WaveAugment(speed_volume_perturb=True, speed_choices=(0.9, 1.0, 1.1))
    fe = front_end(True, wave_augment=wa, rng=np.random.default_rng(5), input_rate=(8000, 16000, 48000))
    got, pct, frames = fe(pack(wavs), lens, rates=rates)
    wd = wa.draw(lens, np.random.default_rng(5), rates=rates)
    assert len(set(wd.speed.tolist())) > 1 and wd.rates.tolist() == [speed_rate(r, s) for r, s in zip(rates, wd.speed.tolist())]
    rows = [Resampler(int(r))(pack([w]), [len(w)]) for w, r in zip(wavs, wd.rates)]
    ns16 = [int(n[0]) for _, n in rows]
    assert ns16 == wd.resampled.tolist()
    wav16 = pack([o[0, :n].cpu().numpy() for (o, _), n in zip(rows, ns16)])
    fe16 = front_end(True, wave_augment=WaveAugment(speed_volume_perturb=True))
    want, wpct, wframes = fe16._call_wave_augmented(wav16, torch.tensor(ns16, dtype=torch.int32), False, wd)
    assert torch.equal(got, want) and torch.equal(pct, wpct) and torch.equal(frames, wframes)
    assert frames.tolist() == [1 + int(n) // HOP for n in wd.nsamples]
    # collate draws in the given order and sorts by the lengths after speed and tempo
    fe = front_end(True, wave_augment=wa, rng=np.random.default_rng(6), input_rate=(8000, 16000, 48000))
    inputs, cpct, order = fe.collate([torch.from_numpy(w) for w in wavs], rates=rates)
    wd = wa.draw(lens, np.random.default_rng(6), rates=rates)
    assert order == sorted(range(6), key=lambda i: -int(wd.nsamples[i]))
    rows = [Resampler(int(wd.rates[i]))(pack([wavs[i]]), [lens[i]]) for i in order]
    ns16 = [int(n[0]) for _, n in rows]
    wav16 = pack([o[0, :n].cpu().numpy() for (o, _), n in zip(rows, ns16)])
    want, wpct, _ = fe16._call_wave_augmented(wav16, torch.tensor(ns16, dtype=torch.int32), False, wd.take(order))
    assert torch.equal(inputs, want) and torch.equal(cpct, wpct)
    # speed alone, on a front-end with one rate: 16 kHz at speed 1.0 is the copy class
    wa1 = WaveAugment(speed_choices=(1.0,))
    fe1 = front_end(True, wave_augment=wa1)
    assert fe1.bank.rates == (16000,) and fe1.bank.half_width == 0
    a = fe1(pack(wavs[:2]), lens[:2])
    b = front_end(True)(pack(wavs[:2]), lens[:2])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 9. the noise bank -----------------------------------------------------------------------------------------------------------
def test_a_noise_bank_of_8_and_44_khz_recordings_equals_the_bank_of_the_converted_recordings():
    from deepspeech.pytorch_amd.augment import NoiseBank
    from deepspeech.pytorch_amd.resample import Resampler
    rates, lens = [8000, 44100, 16000, 8000], [4000, 22050, 5000, 77]
    recs = [clip(500 + k, n, 0.3) for k, n in enumerate(lens)]
    got = NoiseBank.from_waveforms(recs, rates=rates, device=DEV)
    conv = []
    for w, r in zip(recs, rates):
        o, n = Resampler(r)(pack([w]), [len(w)])
        conv.append(o[0, :int(n[0])].cpu().numpy())
    want = NoiseBank.from_waveforms(conv, device=DEV)
    assert got.offsets.tolist() == want.offsets.tolist() and len(got) == 4
    assert [got.length(r) for r in range(4)] == [Resampler(r).out_len(n) for r, n in zip(rates, lens)]
    assert torch.equal(got.samples, want.samples)
    same = NoiseBank.from_waveforms(conv, rates=[16000] * 4, device=DEV)
    assert torch.equal(same.samples, want.samples) and same.offsets.tolist() == want.offsets.tolist()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_the_documented_codes_and_nothing_is_written(real_bank):
    from deepspeech.pytorch_amd import ops
    from deepspeech.pytorch_amd._lib import Ds2HipError, call
    ARG, ALIGN = "1002", "1003"
    wav = pack([clip(1, 100), clip(2, 100)])
    table_dev, taps = real_bank.on(wav.device)
    good = real_bank.classes
    C = len(RATES)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)                      # noqa: E731
    ns, cls = i32([100, 100]), i32([0, 2])
    out = torch.full((2, 200), GARBAGE, device=DEV)
    ns_out = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    state = torch.full((4 * 2 * real_bank.half_width,), GARBAGE, device=DEV)
    ws = torch.full((2 * 2 * real_bank.half_width,), GARBAGE, device=DEV)
    rows = torch.zeros((2, 10), dtype=torch.int32, device=DEV)
    H = lambda t: ctypes.c_void_p(t.ctypes.data)                                        # noqa: E731

    def one_shot_args(**kw):
        a = dict(wav=ops.P(wav), ldw=wav.stride(0), ns=ops.P(ns), cls=ops.P(cls), N=2, host=H(good), dev=ops.P(table_dev), C=C,
                 taps=ops.P(taps), out=ops.P(out), ldo=200, ns_out=ops.P(ns_out))
        a.update(kw)
        return [a[k] for k in ("wav", "ldw", "ns", "cls", "N", "host", "dev", "C", "taps", "out", "ldo", "ns_out")] + [ops.S()]

    def feed_args(**kw):
        a = dict(wav=ops.P(wav), ldw=wav.stride(0), rows=ops.P(rows), n=2, max_new=100, max_emit=200, S=4, host=H(good),
                 dev=ops.P(table_dev), C=C, taps=ops.P(taps), Wmax=real_bank.half_width, state=ops.P(state), out=ops.P(out), ldo=200,
                 ws=ops.P(ws))
        a.update(kw)
        return [a[k] for k in ("wav", "ldw", "rows", "n", "max_new", "max_emit", "S", "host", "dev", "C", "taps", "Wmax", "state", "out",
                               "ldo", "ws")] + [ops.S()]

    big = good.copy()
    big.reshape(-1, WORDS)[1, :3] = (16384, 1, 24)                                      # a table of 3 MiB
    shape = good.copy()
    shape.reshape(-1, WORDS)[0, 5] -= 1                                                 # not the tile shape of the class
    odd = good.copy()
    odd.reshape(-1, WORDS)[2, 8] += 1                                                   # a table on an odd float
    null = ops.P(None)
    for code, kw in ((ARG, dict(wav=null)), (ARG, dict(ns=null)), (ARG, dict(cls=null)), (ARG, dict(dev=null)), (ARG, dict(out=null)),
                     (ARG, dict(ns_out=null)), (ARG, dict(taps=null)), (ARG, dict(out=ops.P(wav))), (ARG, dict(C=0)), (ARG, dict(C=17)),
                     (ARG, dict(host=H(big))), (ARG, dict(host=H(shape))), (ARG, dict(ldw=0)), (ARG, dict(ldo=0)), (ARG, dict(N=0)),
                     (ALIGN, dict(host=H(odd))), (ALIGN, dict(taps=ctypes.c_void_p(taps.data_ptr() + 4)))):
        with pytest.raises(Ds2HipError, match=code):
            call("ds2_resample_mixed", *one_shot_args(**kw))
    for code, kw in ((ARG, dict(rows=null)), (ARG, dict(state=null)), (ARG, dict(ws=null)), (ARG, dict(wav=null)), (ARG, dict(out=null)),
                     (ARG, dict(taps=null)), (ARG, dict(dev=null)), (ARG, dict(S=1)), (ARG, dict(C=17)), (ARG, dict(C=0)),
                     (ARG, dict(host=H(big))), (ARG, dict(ldw=99)), (ARG, dict(ldo=199)), (ARG, dict(Wmax=real_bank.half_width - 1)),
                     (ARG, dict(n=0)), (ALIGN, dict(host=H(odd))), (ALIGN, dict(rows=ctypes.c_void_p(rows.data_ptr() + 4))),
                     (ALIGN, dict(taps=ctypes.c_void_p(taps.data_ptr() + 4)))):
        with pytest.raises(Ds2HipError, match=code):
            call("ds2_resample_stream_feed_mixed", *feed_args(**kw))
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all()) and bool((ns_out == -7).all()) and bool((state == GARBAGE).all()) and bool((ws == GARBAGE).all())
    udw = np.array([(2, 1, 24), (16384, 1, 24)], np.int32)
    tab, total = np.zeros(2 * WORDS, np.int32), ctypes.c_long(0)
    with pytest.raises(Ds2HipError, match=ARG):
        call("ds2_resample_classes", H(udw), 2, H(tab), ctypes.byref(total))
    with pytest.raises(Ds2HipError, match=ARG):
        call("ds2_resample_classes", H(udw), 17, H(tab), ctypes.byref(total))
    with pytest.raises(Ds2HipError, match="no CPU path"):
        real_bank(wav.cpu(), [100, 100], [8000, 8000])
    with pytest.raises(ValueError, match="not a rate of this bank"):
        real_bank(wav, [100, 100], [8000, 22050])
    with pytest.raises(ValueError, match="exceeds"):
        real_bank(wav, [100, 101], [8000, 8000])
