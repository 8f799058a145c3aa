"""CTC forced alignment: where in the audio is each character and each word of a KNOWN transcript.

``ForcedAligner(labels).align(out, sizes, transcripts=[...])`` runs the Viterbi path of every clip's transcript through the
network's outputs on the device (ds2_ctc_align: the CTC lattice with max in place of logsumexp and a trace-back) and returns one
``Alignment`` per clip with the characters' and the words' frame spans.  Uses: cutting long recordings into utterances, flagging
clips whose transcript does not fit the audio (``flag``), subtitles for a transcript that is trusted more than a decode.

The lattice runs on the device; the string-to-label mapping, the grouping of characters into words and the seconds conversion
below are host bookkeeping and import without a GPU (ops, and with it the HIP library, is imported on the first ``align``).
"""
import math
from collections import namedtuple

import torch

KINDS = {"logits": 0, "probs": 1, "log_probs": 2}

# One aligned character or word: frames are inclusive; start_s / end_s are None unless the aligner knows the frame duration
# (start_frame * frame_seconds and (end_frame + 1) * frame_seconds).  span[:4] is (text, start_frame, end_frame, logp).
Span = namedtuple("Span", "text start_frame end_frame logp start_s end_s")
Span.__new__.__defaults__ = (None, None)

# score: log-probability of the best path (-inf when the transcript does not fit); frames: the clip's valid frames;
# frame_labels: int tensor [frames], the label emitted at every frame, blank included (-1 throughout when infeasible)
Alignment = namedtuple("Alignment", "score feasible chars words frame_labels frames")


def labels_to_ints(transcript, char_to_int, blank_index):
    """The label indices of a transcript, through the inverse of the decoders' int_to_char.  ValueError names a character that is
    not a label (or is the blank, which no transcript can contain)."""
    out = []
    for ch in transcript:
        i = char_to_int.get(ch)
        if i is None or i == blank_index:
            raise ValueError("character %r of transcript %r is not one of the labels" % (ch, transcript))
        out.append(i)
    return out


def make_span(text, start_frame, end_frame, logp, frame_seconds=None):
    if frame_seconds is None:
        return Span(text, int(start_frame), int(end_frame), float(logp))
    return Span(text, int(start_frame), int(end_frame), float(logp), int(start_frame) * frame_seconds,
                (int(end_frame) + 1) * frame_seconds)


def group_words(chars, frame_seconds=None, space=' '):
    """Words = maximal runs of non-space characters.  The space closes a word and belongs to none; a word runs from its first
    character's start to its last character's end and its logp is the sum of its characters' logp."""
    words, run = [], []

    def close():
        if run:
            words.append(make_span(''.join(c.text for c in run), run[0].start_frame, run[-1].end_frame,
                                   math.fsum(c.logp for c in run), frame_seconds))
            del run[:]
    for c in chars:
        if c.text == space:
            close()
        else:
            run.append(c)
    close()
    return words


class ForcedAligner:
    def __init__(self, labels, blank_index=0, frame_seconds=None):
        self.labels = labels
        self.blank_index = blank_index
        self.frame_seconds = frame_seconds
        self.int_to_char = dict((i, c) for (i, c) in enumerate(labels))
        self.char_to_int = dict((c, i) for (i, c) in enumerate(labels))

    @classmethod
    def from_model(cls, model):
        """The aligner of a DeepSpeech model: its labels and blank, and the duration of one output frame (the conv stack's time
        stride is 2, so a frame is two spectrogram hops)."""
        return cls(model.labels, blank_index=model.blank_index, frame_seconds=2 * model.spect_cfg.window_stride)

    def targets_of(self, transcripts):
        """(flat int32 targets, int32 target_sizes) of a list of transcript strings."""
        ints = [labels_to_ints(s, self.char_to_int, self.blank_index) for s in transcripts]
        flat = [i for t in ints for i in t]
        return torch.tensor(flat, dtype=torch.int32), torch.tensor([len(t) for t in ints], dtype=torch.int32)

    def spans(self, target, tok_start, tok_end, tok_logp):
        """chars and words of one clip from its labels and their aligned frames (host lists)."""
        chars = [make_span(self.int_to_char[int(c)], s, e, lp, self.frame_seconds)
                 for c, s, e, lp in zip(target, tok_start, tok_end, tok_logp)]
        return chars, group_words(chars, self.frame_seconds)

    def align(self, out, sizes, transcripts=None, targets=None, target_sizes=None, kind="probs"):
        """out: (N, T', C) device tensor as DeepSpeech.forward returns it -- probabilities in eval mode (kind="probs"), logits in
        training mode ("logits"), or "log_probs"; sizes: [N] valid frames.  The transcript of every clip is given either as
        strings (transcripts) or as the flat integer targets of a batch with target_sizes.  Returns [Alignment] per clip."""
        from . import ops
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
        if (transcripts is None) == (targets is None):
            raise ValueError("give the transcripts either as strings (transcripts) or as targets with target_sizes")
        if transcripts is not None:
            targets, target_sizes = self.targets_of(transcripts)
        elif target_sizes is None:
            raise ValueError("targets need target_sizes")
        tgt = torch.as_tensor(targets).reshape(-1).cpu()
        tsz = torch.as_tensor(target_sizes).reshape(-1).cpu()
        if out.dtype != torch.float32:
            out = out.float()
        fs, ts, te, tl, score = ops.ctc_align(out, sizes, tgt, tsz, blank=self.blank_index, mode=KINDS[kind])
        fs, ts, te, tl, score = fs.cpu(), ts.tolist(), te.tolist(), tl.tolist(), score.tolist()
        frames = torch.as_tensor(sizes).reshape(-1).tolist()
        tgt_l, res, off = tgt.tolist(), [], 0
        for n, L in enumerate(tsz.tolist()):
            target, T = tgt_l[off:off + L], max(0, min(int(frames[n]), out.shape[1]))
            feasible = score[n] != float("-inf")
            st = fs[n, :T].long()
            if feasible:
                chars, words = self.spans(target, ts[off:off + L], te[off:off + L], tl[off:off + L])
                ext = torch.full((2 * L + 1,), self.blank_index, dtype=torch.int32)
                ext[1::2] = torch.tensor(target, dtype=torch.int32)
                frame_labels = ext[st]
            else:
                chars, words, frame_labels = [], [], torch.full((T,), -1, dtype=torch.int32)
            res.append(Alignment(score[n], feasible, chars, words, frame_labels, T))
            off += L
        return res

    @staticmethod
    def flag(alignments, min_mean_logp):
        """Indices of the clips whose transcript does not fit the audio: no path at all, or a mean log-probability per frame
        (score / frames) below min_mean_logp."""
        return [i for i, a in enumerate(alignments)
                if not a.feasible or a.frames == 0 or a.score / a.frames < min_mean_logp]
