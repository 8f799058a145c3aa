"""Sample-rate conversion to the front-end's 16 kHz on the device (csrc/ds2_resample.hip): a rational
polyphase filter, one-shot over a ragged batch and streamed over slots, the streamed samples equal to the one-shot ones bit for
bit however the audio is cut into feeds.  The reference converts its corpora with sox ``rate`` in offline data scripts; this is
the project's own windowed-sinc design, as the tempo change is the project's own WSOLA.

    g = gcd(in_rate, 16000), U = 16000 / g, D = in_rate / g, r = min(1, U / D), W = ceil(zeros / r)
    h[p][j] = c sinc(c t) I0(beta sqrt(1 - (t / W)^2)) / I0(beta),  t = (j - W + 1) - p / U,  c = r rolloff   (0 where |t| > W)
    every phase divided by its own sum, then rounded once to float32
    y[m] = sum_j h[p][j] x[n0 - W + 1 + j],  n0 = floor(m D / U),  p = (m D) mod U,  x = 0 outside the clip,  m < ceil(n U / D)

The taps are built here in float64 and only here; the kernels take the table as an argument.

``ResamplerBank`` puts up to 16 such designs behind one launch, the rate belonging to the row: batches and pools that mix rates,
speed perturbation by resampling (``augment.WaveAugment(speed_choices=...)``) and noise recordings at other rates go through it."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import ops
from ._lib import Ds2HipError, call, query

OUT_RATE = 16000
MAX_TABLE_BYTES = 128 * 1024
RESAMPLE_ROW_WORDS = 10    # int32 words of one ds2_resample_stream_row: slot, src, carried, n_new, out_before (2), emit, final, fresh, pad
_ROW_STAGING = ops.PinnedRing()

ResamplePlan = collections.namedtuple("ResamplePlan", "out_before emit carried new_carry first")


def design_taps(up, down, zeros=24, rolloff=0.92, beta=9.0):
    """(half_width W, taps [up][2W] float32) of the Kaiser-windowed sinc above, computed in float64."""
    U, D = int(up), int(down)
    r = min(1.0, U / D)
    W = int(zeros) if D <= U else -((-int(zeros) * D) // U)
    p = np.arange(U, dtype=np.float64)[:, None]
    j = np.arange(2 * W, dtype=np.float64)[None, :]
    t = (j - W + 1) - p / U
    c = r * float(rolloff)
    inside = np.abs(t) <= W
    win = np.i0(float(beta) * np.sqrt(np.clip(1.0 - (t / W) ** 2, 0.0, None))) / np.i0(float(beta))
    h = np.where(inside, c * np.sinc(c * t) * win, 0.0)
    h /= h.sum(axis=1, keepdims=True)
    return W, h.astype(np.float32)


class Resampler:
    def __init__(self, in_rate, out_rate=OUT_RATE, zeros=24, rolloff=0.92, beta=9.0):
        """in_rate: any positive integer rate in Hz whose table up * 2 half_width * 4 bytes is at most 128 KiB (8000, 11025, 22050,
        24000, 32000, 44100, 48000 ... all are); 16000 is the identity: no kernel runs.  out_rate: the front-end's 16000, the only
        one built.  zeros / rolloff / beta: zero crossings of the sinc per side at the lower rate, the cut-off as a fraction of the
        lower Nyquist frequency, the Kaiser window's beta."""
        if int(in_rate) != in_rate or int(in_rate) <= 0:
            raise ValueError("in_rate must be a positive integer number of Hz, got %r" % (in_rate,))
        if int(out_rate) != OUT_RATE:
            raise ValueError("the resampler feeds the 16 kHz front-end: out_rate must be %d, got %r" % (OUT_RATE, out_rate))
        if int(zeros) < 1 or not 0.0 < float(rolloff) <= 1.0 or not float(beta) >= 0.0:
            raise ValueError("zeros must be >= 1, rolloff in (0, 1] and beta >= 0, got %r, %r, %r" % (zeros, rolloff, beta))
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        g = math.gcd(self.in_rate, self.out_rate)
        self.up, self.down = self.out_rate // g, self.in_rate // g
        self.identity = self.in_rate == self.out_rate
        self._dev_taps = {}
        if self.identity:
            self.half_width, self.taps = 0, np.zeros((1, 0), np.float32)
            return
        W = int(zeros) if self.down <= self.up else -((-int(zeros) * self.down) // self.up)
        nbytes = self.up * 2 * W * 4
        if nbytes > MAX_TABLE_BYTES:
            raise ValueError("%d Hz -> %d Hz needs U = %d phases of 2W = %d taps (D = %d): a table of %d bytes, over the %d the "
                             "kernels take" % (self.in_rate, self.out_rate, self.up, 2 * W, self.down, nbytes, MAX_TABLE_BYTES))
        self.half_width, self.taps = design_taps(self.up, self.down, zeros, rolloff, beta)
        assert self.half_width == W

    def taps_on(self, dev):
        """the table on `dev`, uploaded once per device"""
        dev = torch.device(dev)
        t = self._dev_taps.get(dev)
        if t is None:
            t = self._dev_taps[dev] = torch.from_numpy(self.taps).to(dev)
        return t

    def out_len(self, n):
        """ds2_resample_out_len: ceil(n up / down) output samples of n input samples"""
        n = int(n)
        if n < 0:
            raise ValueError("out_len: n must be >= 0")
        return -((-n * self.up) // self.down)

    def plan_resample(self, samples_before, n_new, final=False):
        """ds2_resample_plan: after `samples_before` input samples of a stream, a feed of `n_new` more (final: the utterance ends
        with it).  G samples of a stream that goes on complete E(G) = 0 for G <= W, else ceil((G - W) U / D) outputs -- those whose
        last tap n0 + W has arrived -- and the end completes out_len(G); the feed emits the difference.  `carried` samples in front
        of the new ones come from the slot (those from `first` = max(0, n0(out_before) - W + 1) on), `new_carry` <= 2W - 1 stay
        for the next feed (0 after a final one)."""
        G0, n = int(samples_before), int(n_new)
        if G0 < 0 or n < 0:
            raise ValueError("plan_resample: samples_before and n_new must be >= 0")
        U, D, W = self.up, self.down, self.half_width
        if self.identity:
            return ResamplePlan(G0, n, 0, 0, G0)

        def outputs(G, fin):
            return -((-G * U) // D) if fin else (0 if G <= W else -((-(G - W) * U) // D))

        def first_input(m):
            return max(0, (m * D) // U - W + 1)

        G1 = G0 + n
        e0, e1 = outputs(G0, False), outputs(G1, final)
        first = first_input(e0)
        return ResamplePlan(e0, e1 - e0, G0 - first, 0 if final else G1 - first_input(e1), first)

    def _run(self, wav, ns):
        """wav (N, Lmax) f32 on the device, ns [N] int32 on the host, checked by the caller -> (wav16 (N, max out_len), its sample
        counts on the device (written by the kernel), the same counts on the host (closed form: nothing is read back))."""
        ns16 = torch.tensor([self.out_len(v) for v in ns.tolist()], dtype=torch.int32)
        out, ns_dev = ops.resample(wav, ns, self.taps_on(wav.device), self.up, self.down, self.half_width, int(ns16.max()))
        return out, ns_dev, ns16

    def __call__(self, wav, nsamples):
        """wav: [N][Lmax] float32 on a HIP device (row n = clip n), nsamples: [N] ints >= 1.  Returns (wav16 (N, max out_len) on the
        device, zero beyond a clip's own samples; nsamples16 [N] int32 on the host)."""
        if not wav.is_cuda:
            raise Ds2HipError("Resampler needs the waveforms on a HIP device; there is no CPU path")
        ns = torch.as_tensor(nsamples, dtype=torch.int32).cpu().reshape(-1)
        if wav.dim() != 2 or ns.numel() != wav.shape[0] or int(ns.min()) < 1:
            raise ValueError("expected a [N][Lmax] waveform batch and one positive sample count per row")
        if int(ns.max()) > wav.shape[1]:
            raise ValueError("nsamples exceeds the waveform buffer")
        wav = wav.float().contiguous()
        if self.identity:
            return wav, ns
        out, _, ns16 = self._run(wav, ns)
        return out, ns16

    def stream(self, capacity, device):
        """A streaming handle over `capacity` slots (``ResampleStream``): audio fed in chunks of any lengths gives the samples of
        the one-shot call on the whole clip, bit for bit."""
        return ResampleStream(self, capacity, device)


class ResampleStream:
    """The streaming form of a ``Resampler`` (ds2_resample_stream_feed): per slot the device keeps the at most 2W - 1 input samples
    that outputs not yet complete need; the host keeps the input sample count, from which every count of a feed follows in closed
    form (``Resampler.plan_resample``), so nothing is read back."""

    def __init__(self, resampler, capacity, device):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %s" % (capacity,))
        self.resampler, self.capacity, self.device = resampler, int(capacity), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        S = self.capacity
        self._state = None              # the carries [S][2W] f32, allocated by the first feed
        self.samples, self.ended, self._fresh = [0] * S, [False] * S, [True] * S       # samples: INPUT samples fed so far

    def reset(self, slots=None):
        """These slots (None = all) start a new stream: their carry reads as empty from the next feed on; nothing is launched."""
        for s in (range(self.capacity) if slots is None else [int(v) for v in slots]):
            if not 0 <= s < self.capacity:
                raise ValueError("slot %d is not a slot of this stream (capacity %d)" % (s, self.capacity))
            self.samples[s], self.ended[s], self._fresh[s] = 0, False, True

    def feed(self, slots, wav, nsamples, final=()):
        """wav: [len(slots)][L] float32 on the device, row i = the nsamples[i] >= 0 new input samples of slots[i]; final: the slots
        whose utterance ends with this feed.  Returns (wav16 (len(slots), Lc) float32 with Lc the largest count of new output
        samples -- possibly 0 --, counts [len(slots)] ints): row i holds counts[i] new samples, zero beyond them."""
        rs, S = self.resampler, self.capacity
        sl, fin = [int(s) for s in slots], set(int(s) for s in final)
        if not sl or len(set(sl)) != len(sl) or any(not 0 <= s < S for s in sl):
            raise ValueError("slots must be distinct and lie in [0, %d), got %s" % (S, sl))
        if not fin <= set(sl):
            raise ValueError("final names slots that are not in this feed: %s" % sorted(fin - set(sl)))
        ns = [int(v) for v in nsamples]
        if wav.dim() != 2 or wav.shape[0] != len(sl) or len(ns) != len(sl) or any(v < 0 or v > wav.shape[1] for v in ns):
            raise ValueError("expected a [%d][L] waveform chunk and %d sample counts in [0, L], got %s and %s"
                             % (len(sl), len(sl), tuple(wav.shape), ns))
        for s in sl:
            if self.ended[s]:
                raise ValueError("the stream of slot %d has ended (a final feed); reset it first" % s)
        if not wav.is_cuda or wav.device != self.device:
            raise Ds2HipError("ResampleStream needs the waveforms on %s; there is no CPU path" % self.device)
        wav = wav.float()
        if wav.shape[1] and wav.stride(1) != 1:
            wav = wav.contiguous()
        if rs.identity:
            out, counts = wav, ns
        else:
            plans = [rs.plan_resample(self.samples[s], n, s in fin) for s, n in zip(sl, ns)]
            assert all(self.samples[s] == 0 for s in sl if self._fresh[s]) and all(0 <= p.new_carry < 2 * rs.half_width for p in plans)
            table = np.zeros((len(sl), RESAMPLE_ROW_WORDS), dtype=np.int32)
            for i, (s, n, p) in enumerate(zip(sl, ns, plans)):
                table[i, :4] = (s, i, 0 if self._fresh[s] else p.carried, n)
                table[i, 4:6] = np.array([p.out_before], dtype=np.int64).view(np.int32)
                table[i, 6:9] = (p.emit, int(s in fin), int(self._fresh[s]))
            counts = [p.emit for p in plans]
            if self._state is None:
                self._state = torch.zeros(query("ds2_resample_stream_state_bytes", S, rs.half_width), dtype=torch.uint8, device=self.device)
            rows = _ROW_STAGING.stage(self.device, [table.reshape(-1)])
            out = ops.resample_stream_feed(wav, rows, len(sl), max(ns), max(counts), S, rs.taps_on(self.device), rs.up, rs.down,
                                           rs.half_width, self._state)
        for s, n in zip(sl, ns):
            self.samples[s] += n
            self.ended[s], self._fresh[s] = s in fin, False
        return out, counts


MAX_CLASSES = 16
CLASS_WORDS = 10           # int32 words of one ds2_resample_class: U, D, W, nt, P, K, tile, cap, taps_off (2)


class ResamplerBank:
    """Up to 16 input rates behind one launch (ds2_resample_mixed; DESIGN.md section 7.2, "Mixed rates"): rate, half-width and tap
    table belong to the row.  Class c is ``Resampler(rates[c])``'s design -- the same ``design_taps`` call, so the same bits -- and a
    row of a mixed call equals that resampler's call on the clip alone, bit for bit.  16000 is the copy class: its rows ride in
    the same launch and come out as they went in."""

    def __init__(self, rates, zeros=24, rolloff=0.92, beta=9.0):
        rates = list(rates)
        if not rates or any(int(r) != r or int(r) <= 0 for r in rates):
            raise ValueError("rates must be positive integer numbers of Hz, got %r" % (rates,))
        rates = [int(r) for r in rates]
        if len(set(rates)) != len(rates):
            raise ValueError("rates must be distinct, got %r" % (rates,))
        if len(rates) > MAX_CLASSES:
            raise ValueError("a bank holds at most %d rates, got %d: %r" % (MAX_CLASSES, len(rates), rates))
        self.rates = tuple(rates)
        self.resamplers = [Resampler(r, zeros=zeros, rolloff=rolloff, beta=beta) for r in rates]   # refuses an oversized table, naming the rate
        self.class_of = {r: c for c, r in enumerate(rates)}
        self.half_width = max(rs.half_width for rs in self.resamplers)
        C_ = len(rates)
        udw = np.array([(rs.up, rs.down, rs.half_width) for rs in self.resamplers], dtype=np.int32)
        self.classes = np.zeros(C_ * CLASS_WORDS, dtype=np.int32)
        total = ctypes.c_long(0)
        call("ds2_resample_classes", ctypes.c_void_p(udw.ctypes.data), C_, ctypes.c_void_p(self.classes.ctypes.data), ctypes.byref(total))
        self.taps = np.concatenate([rs.taps.reshape(-1) for rs in self.resamplers]).astype(np.float32)
        offs = self.classes.reshape(C_, CLASS_WORDS)[:, 8:10].copy().view(np.int64).reshape(-1)
        assert self.taps.size == total.value and offs.tolist() == np.cumsum([0] + [rs.taps.size for rs in self.resamplers])[:-1].tolist()
        self._dev = {}

    def tile(self, rate):
        """the consecutive outputs one workgroup of a one-shot launch computes for a row at `rate`"""
        return int(self.classes.reshape(-1, CLASS_WORDS)[self._class(rate), 6])

    def _class(self, rate):
        c = self.class_of.get(int(rate)) if int(rate) == rate else None
        if c is None:
            raise ValueError("%r Hz is not a rate of this bank %r" % (rate, self.rates))
        return c

    def resampler(self, rate):
        return self.resamplers[self._class(rate)]

    def out_len(self, n, rate):
        return self.resampler(rate).out_len(n)

    def plan_resample(self, rate, samples_before, n_new, final=False):
        return self.resampler(rate).plan_resample(samples_before, n_new, final)

    def on(self, dev):
        """(class table, taps) on `dev`, uploaded once per device"""
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = (torch.from_numpy(self.classes).to(dev), torch.from_numpy(self.taps).to(dev) if self.taps.size else None)
        return t

    def _run(self, wav, ns, rates):
        """wav (N, Lmax) f32 on the device, ns [N] int32 on the host, rates: one of the bank per row, all checked by the caller ->
        (wav16, its sample counts on the device, the same counts on the host in closed form).  One staged upload, one launch."""
        cls = [self._class(r) for r in rates]
        ns16 = torch.tensor([self.resamplers[c].out_len(v) for c, v in zip(cls, ns.tolist())], dtype=torch.int32)
        N = len(cls)
        up = _ROW_STAGING.stage(wav.device, [ns.numpy().astype(np.int32), np.asarray(cls, dtype=np.int32)])
        classes_dev, taps = self.on(wav.device)
        out, ns_dev = ops.resample_mixed(wav, up[:N], up[N:], self.classes, classes_dev, taps, int(ns16.max()))
        return out, ns_dev, ns16

    def __call__(self, wav, nsamples, rates):
        """wav: [N][Lmax] float32 on a HIP device, nsamples: [N] ints >= 1, rates: [N] rates of the bank, the rate of each row.
        Returns (wav16 (N, max out_len) on the device, zero beyond a clip's own samples; nsamples16 [N] int32 on the host)."""
        if not wav.is_cuda:
            raise Ds2HipError("ResamplerBank needs the waveforms on a HIP device; there is no CPU path")
        ns = torch.as_tensor(nsamples, dtype=torch.int32).cpu().reshape(-1)
        rates = list(rates)
        if wav.dim() != 2 or ns.numel() != wav.shape[0] or len(rates) != wav.shape[0] or int(ns.min()) < 1:
            raise ValueError("expected a [N][Lmax] waveform batch, one positive sample count and one rate per row")
        if int(ns.max()) > wav.shape[1]:
            raise ValueError("nsamples exceeds the waveform buffer")
        out, _, ns16 = self._run(wav.float().contiguous(), ns, rates)
        return out, ns16

    def stream(self, capacity, device):
        """A streaming handle over `capacity` slots, each at a rate of its own (``BankStream``)."""
        return BankStream(self, capacity, device)


class BankStream:
    """The streaming form of a ``ResamplerBank`` (ds2_resample_stream_feed_mixed): ``ResampleStream`` with a rate per slot, given
    by ``reset(slots, rates)`` for the stream that starts; slots at different rates advance in one feed."""

    def __init__(self, bank, capacity, device):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1, got %s" % (capacity,))
        self.bank, self.capacity, self.device = bank, int(capacity), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        S = self.capacity
        self._wmax = max(bank.half_width, 1)
        self._state = None              # the carries [S][2 Wmax] f32, allocated by the first feed
        self.samples, self.ended, self._fresh, self.rates = [0] * S, [False] * S, [True] * S, [None] * S

    def reset(self, slots=None, rates=None):
        """These slots (None = all) start a new stream at rates[i] (one rate: all of them; None: the rate each had).  Their carry
        reads as empty from the next feed on; nothing is launched."""
        sl = list(range(self.capacity)) if slots is None else [int(v) for v in slots]
        if rates is not None and not isinstance(rates, (list, tuple)):
            rates = [rates] * len(sl)
        if rates is not None and len(rates) != len(sl):
            raise ValueError("reset: %d rates for %d slots" % (len(rates), len(sl)))
        for s in sl:
            if not 0 <= s < self.capacity:
                raise ValueError("slot %d is not a slot of this stream (capacity %d)" % (s, self.capacity))
        if rates is not None:
            rates = [self.bank.rates[self.bank._class(r)] for r in rates]
        for i, s in enumerate(sl):
            self.samples[s], self.ended[s], self._fresh[s] = 0, False, True
            if rates is not None:
                self.rates[s] = rates[i]

    def feed(self, slots, wav, nsamples, final=()):
        """As ``ResampleStream.feed``; row i is at the rate of slots[i]."""
        bank, S = self.bank, self.capacity
        sl, fin = [int(s) for s in slots], set(int(s) for s in final)
        if not sl or len(set(sl)) != len(sl) or any(not 0 <= s < S for s in sl):
            raise ValueError("slots must be distinct and lie in [0, %d), got %s" % (S, sl))
        if not fin <= set(sl):
            raise ValueError("final names slots that are not in this feed: %s" % sorted(fin - set(sl)))
        ns = [int(v) for v in nsamples]
        if wav.dim() != 2 or wav.shape[0] != len(sl) or len(ns) != len(sl) or any(v < 0 or v > wav.shape[1] for v in ns):
            raise ValueError("expected a [%d][L] waveform chunk and %d sample counts in [0, L], got %s and %s"
                             % (len(sl), len(sl), tuple(wav.shape), ns))
        for s in sl:
            if self.rates[s] is None:
                raise ValueError("slot %d has no rate yet: reset(slots, rates) gives it one" % s)
            if self.ended[s]:
                raise ValueError("the stream of slot %d has ended (a final feed); reset it first" % s)
        if not wav.is_cuda or wav.device != self.device:
            raise Ds2HipError("BankStream needs the waveforms on %s; there is no CPU path" % self.device)
        wav = wav.float()
        if wav.shape[1] and wav.stride(1) != 1:
            wav = wav.contiguous()
        cls = [bank.class_of[self.rates[s]] for s in sl]
        plans = [bank.resamplers[c].plan_resample(self.samples[s], n, s in fin) for c, s, n in zip(cls, sl, ns)]
        assert all(self.samples[s] == 0 for s in sl if self._fresh[s])
        assert all(0 <= p.new_carry < max(2 * bank.resamplers[c].half_width, 1) for c, p in zip(cls, plans))
        table = np.zeros((len(sl), RESAMPLE_ROW_WORDS), dtype=np.int32)
        for i, (s, n, p, c) in enumerate(zip(sl, ns, plans, cls)):
            copy = bank.resamplers[c].identity            # the copy class has no carry and counts no outputs before
            table[i, :4] = (s, i, 0 if self._fresh[s] or copy else p.carried, n)
            table[i, 4:6] = np.array([0 if copy else p.out_before], dtype=np.int64).view(np.int32)
            table[i, 6:10] = (p.emit, int(s in fin), int(self._fresh[s]), c)
        counts = [p.emit for p in plans]
        if self._state is None:
            self._state = torch.zeros(query("ds2_resample_stream_state_bytes_mixed", S, self._wmax), dtype=torch.uint8, device=self.device)
        rows = _ROW_STAGING.stage(self.device, [table.reshape(-1)])
        classes_dev, taps = bank.on(self.device)
        out = ops.resample_stream_feed_mixed(wav, rows, len(sl), max(ns), max(counts), S, bank.classes, classes_dev, taps, self._wmax,
                                             self._state)
        for s, n in zip(sl, ns):
            self.samples[s] += n
            self.ended[s], self._fresh[s] = s in fin, False
        return out, counts
