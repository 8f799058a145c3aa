"""Keyword spotting on saved network outputs: where in which clip was one of these phrases said
(deepspeech.pytorch_amd.keywords.KeywordSpotter on the device).

    python tools/spot_keywords.py --keyword "HEY THERE" --keyword " STOP :-0.5" [--threshold -1.0] [--hold 25] batch0.npz ...

Each .npz holds one batch, the same files tools/align.py reads: probs (N, T', C) probabilities and sizes (N) valid frames (other
arrays are ignored).  A keyword is a string over the labels; a trailing ":<number>" gives it a threshold of its own (nats per
label).  The JSON holds, per clip in the order of the files, frames, detections as {keyword, start_frame, end_frame, start_s,
end_s, score, score_per_label}, dropped (hits beyond --max-hits per keyword) and, with --best, the largest score of every keyword
whatever the threshold, from which a threshold can be chosen.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech.pytorch_amd.configs import LABELS  # noqa: E402
from deepspeech.pytorch_amd.keywords import KeywordSpotter  # noqa: E402


def parse_keyword(text):
    """"PHRASE" or "PHRASE:threshold" (the last colon splits, when what follows is a number)"""
    head, sep, tail = text.rpartition(":")
    if sep:
        try:
            return head, float(tail)
        except ValueError:
            pass
    return text


def _finite(v):
    return v if v == v and abs(v) != float("inf") else None


def main(argv=None):
    ap = argparse.ArgumentParser(description="Keyword spotting on saved outputs (CTC keyword lattice on the device)")
    ap.add_argument("batches", nargs="+", help=".npz files with probs and sizes")
    ap.add_argument("--keyword", action="append", required=True, help="a phrase over the labels, optionally PHRASE:threshold")
    ap.add_argument("--output-path", default="keywords.json")
    ap.add_argument("--labels-path", default=None, help="JSON list of labels (default: the package's labels)")
    ap.add_argument("--frame-seconds", type=float, default=0.02, help="duration of one output frame")
    ap.add_argument("--threshold", type=float, default=-1.0, help="nats per label (a definition, not a calibrated value)")
    ap.add_argument("--hold", type=int, default=25, help="frames a candidate waits for a better end")
    ap.add_argument("--max-hits", type=int, default=8, help="hits kept per keyword and clip")
    ap.add_argument("--best", action="store_true", help="also write every keyword's largest score per clip")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "spot_keywords needs a HIP device"
    labels = LABELS
    if a.labels_path:
        with open(a.labels_path) as f:
            labels = json.load(f)
    sp = KeywordSpotter(labels, [parse_keyword(k) for k in a.keyword], threshold=a.threshold, hold=a.hold,
                        blank_index=labels.index('_') if '_' in labels else 0, frame_seconds=a.frame_seconds, max_hits=a.max_hits)
    clips = []
    for path in a.batches:
        with np.load(path) as z:
            probs, sizes = torch.from_numpy(z["probs"]).cuda(), torch.from_numpy(z["sizes"])
        dets, best = sp.spot(probs, sizes, kind="probs", return_best=True)
        for n, found in enumerate(dets):
            clip = {"frames": int(sizes[n]), "dropped": sp.last_dropped[n],
                    "detections": [{"keyword": d.keyword, "start_frame": d.start_frame, "end_frame": d.end_frame, "start_s": d.start_s,
                                    "end_s": d.end_s, "score": d.score, "score_per_label": d.score_per_label} for d in found]}
            if a.best:
                clip["best"] = [{"keyword": b.keyword, "score": _finite(b.score), "score_per_label": _finite(b.score_per_label),
                                 "start_frame": b.start_frame, "end_frame": b.end_frame} for b in best[n]]
            clips.append(clip)
    with open(a.output_path, "w") as f:
        json.dump({"frame_seconds": a.frame_seconds, "keywords": sp.keywords, "thresholds": sp.thresholds, "hold": sp.hold,
                   "clips": clips}, f, indent=1)
    print("%d clips, %d detections -> %s" % (len(clips), sum(len(c["detections"]) for c in clips), a.output_path))


if __name__ == "__main__":
    main()
