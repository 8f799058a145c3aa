"""fp64 restatement of exact chunked inference on the oracle's own functions: conv2d_fwd with zero time
padding on explicit windows, bn_eval_fwd, hardtanh_fwd, batch_rnn_fwd with h0 and the lookahead sum.  Between feeds it keeps the
stated carries only -- the last 10 input frames, the last 10 conv1 activations, the last ctx - 1 RNN rows and the hidden state --
and the index plan is streaming.plan_feed's.  The window functions are also what the kernel-level GPU tests compare with."""
import numpy as np

from oracle import ds2_oracle as O
from deepspeech.pytorch_amd.streaming import plan_feed

K = 10


def window(carry, chunk, lens, axis):
    """[carry | chunk] along `axis` with every stream's positions beyond K + lens[n] zeroed (stream axis: 0 for the (N, C, F, T)
    conv windows, 1 for the (T, N, H) row window), and the next carry V[lens[n] : lens[n] + K] per stream."""
    v = np.concatenate([carry, chunk], axis=axis)
    k = carry.shape[axis]
    nxt = np.zeros_like(carry)
    for n, ln in enumerate(lens):
        if axis == 3:
            v[n, :, :, k + ln:] = 0
            nxt[n] = v[n, :, :, ln:ln + k]
        else:
            v[k + ln:, n] = 0
            nxt[:, n] = v[ln:ln + k, n]
    return v, nxt


def _slice_time(v, start, count):
    """`count` positions of the window from `start` on, zero beyond its end"""
    out = np.zeros(v.shape[:3] + (count,), dtype=v.dtype)
    m = max(min(v.shape[3] - start, count), 0)
    out[..., :m] = v[..., start:start + m]
    return out


def conv_window(v, off, J, w, b, gamma, beta, rmean, rvar, stride_t, live):
    """J frames of conv + eval BatchNorm + Hardtanh whose frame j reads window positions off + stride_t * j .. + 10; frames
    j >= live[n] zero.  (N, 32, F_out, J)."""
    N = v.shape[0]
    if J == 0:
        return np.zeros((N, w.shape[0], O._out_size(v.shape[2], w.shape[2], 2, w.shape[2] // 2), 0), dtype=v.dtype)
    y = O.conv2d_fwd(_slice_time(v, off, stride_t * (J - 1) + 11), w, b, (2, stride_t), (w.shape[2] // 2, 0))
    assert y.shape[3] == J
    a = O.hardtanh_fwd(O.bn_eval_fwd(y, gamma, beta, rmean, rvar, 1))
    for n in range(N):
        a[n, :, :, int(live[n]):] = 0
    return a


def lookahead_window(v, off, J, w):
    """J rows hardtanh(sum_k w[h][k] * V[off + t + k]) of the row window v (T, N, H); w (H, 1, ctx)"""
    ctx = w.shape[2]
    vp = np.concatenate([v, np.zeros((off + J + ctx,) + v.shape[1:], v.dtype)], axis=0)
    y = np.zeros((J,) + v.shape[1:], v.dtype)
    for k in range(ctx):
        y += vp[off + k:off + k + J] * w[:, 0, k][None, None, :]
    return O.hardtanh_fwd(y)


class ChunkedReference:
    def __init__(self, P, cfg, N, F0=161):
        self.P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
        self.cfg, self.N, self.F0 = cfg, N, F0
        self.ctx = cfg["lookahead_context"]
        H = cfg["hidden_size"]
        F1 = O._out_size(F0, 41, 2, 20)
        self.c_in, self.c_act = np.zeros((N, 1, F0, K)), np.zeros((N, 32, F1, K))
        self.c_la = np.zeros((self.ctx - 1, N, H))
        self.hs, self.fed, self.plans = None, 0, []

    def feed(self, x, lens, final=False):
        """x (N, 1, F0, Tc), lens [N]; returns (probabilities (N, J3, C), valid frames per stream)"""
        P, N, ctx = self.P, self.N, self.ctx
        lens = [int(v) for v in lens]
        chunk = max(lens) if lens else 0
        p = plan_feed(self.fed, chunk, ctx, final)
        self.plans.append(p)
        J1, J2, J3 = p.j1_new - p.j1_old, p.j2_new - p.j2_old, p.j3_new - p.j3_old
        if final:
            tot = [(self.fed + v - 1) // 2 + 1 if self.fed + v > 0 else 0 for v in lens]
        else:
            assert all(v == x.shape[3] for v in lens)
            tot = [p.j1_new + p.j2_new + p.j3_new] * N             # beyond every range: nothing is masked
        clip = lambda lo, J: [min(max(t - lo, 0), J) for t in tot]
        sm = "conv.seq_module."
        v, self.c_in = window(self.c_in, np.asarray(x, dtype=np.float64), lens, 3)
        a1 = conv_window(v, p.off1, J1, P[sm + "0.weight"], P[sm + "0.bias"], P[sm + "1.weight"], P[sm + "1.bias"],
                         P[sm + "1.running_mean"], P[sm + "1.running_var"], 2, clip(p.j1_old, J1))
        v, self.c_act = window(self.c_act, a1, [J1] * N, 3)
        a2 = conv_window(v, p.off2, J2, P[sm + "3.weight"], P[sm + "3.bias"], P[sm + "4.weight"], P[sm + "4.bias"],
                         P[sm + "4.running_mean"], P[sm + "4.running_var"], 1, clip(p.j2_old, J2))
        self.fed += chunk
        if J2 == 0:
            return np.zeros((N, 0, P["fc.0.module.1.weight"].shape[0])), [0] * N
        xr = a2.reshape(N, -1, J2).transpose(2, 0, 1).copy()       # feature index c*F2 + f, (T, N, H)
        new_hs = []
        for l in range(self.cfg["hidden_layers"]):
            xr, hn, _ = O.batch_rnn_fwd(P, "rnns.%d" % l, self.cfg["rnn_type"], xr, np.asarray(clip(p.j2_old, J2)), False,
                                        batch_norm=(l > 0), train=False, h0=None if self.hs is None else self.hs[l])
            new_hs.append(hn)
        self.hs = new_hs
        v, self.c_la = window(self.c_la, xr, [J2] * N, 0)
        if J3 == 0:
            return np.zeros((N, 0, P["fc.0.module.1.weight"].shape[0])), [0] * N
        y = lookahead_window(v, p.off3, J3, P["lookahead.0.conv.weight"])
        flat = O.bn_eval_fwd(y.reshape(J3 * N, -1), P["fc.0.module.0.weight"], P["fc.0.module.0.bias"],
                             P["fc.0.module.0.running_mean"], P["fc.0.module.0.running_var"], 1)
        out = (flat @ P["fc.0.module.1.weight"].T).reshape(J3, N, -1).transpose(1, 0, 2)
        e = np.exp(out - out.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True), clip(p.j3_old, J3)


def stream_all(P, cfg, x, lengths, chunks, F0=161):
    """Feeds x (N, 1, F0, T) in `chunks` (input frames per feed, the last one final and ragged by `lengths`).  Returns the emitted
    probabilities per stream, concatenated over the feeds ([N] arrays (frames, C)), and the reference object."""
    N = x.shape[0]
    ref = ChunkedReference(P, cfg, N, F0)
    got, pos = [[] for _ in range(N)], 0
    for i, c in enumerate(chunks):
        last = i == len(chunks) - 1
        lens = [min(max(int(g) - pos, 0), c) for g in lengths] if last else [c] * N
        probs, sizes = ref.feed(x[:, :, :, pos:pos + c], lens, final=last)
        for n in range(N):
            got[n].append(probs[n, :sizes[n]])
        pos += c
    return [np.concatenate(g, axis=0) for g in got], ref
