"""Forced alignment of saved network outputs with their reference transcripts: word timings and a list of clips whose transcript
does not fit the audio (deepspeech.pytorch_amd.align.ForcedAligner on the device).

    python tools/align.py --output-path align.json [--min-mean-logp -2.5] batch0.npz batch1.npz ...

Each .npz holds one batch, the same files tools/search_lm_params.py reads: probs (N, T', C) probabilities, sizes (N) valid frames,
targets (the references' labels back to back) and target_sizes (N).  The JSON holds, per clip in the order of the files, score,
feasible, frames and words as {word, start_frame, end_frame, start_s, end_s, logp}; with --min-mean-logp also "flagged", the
indices of the clips that are infeasible or whose score per frame is below the bar.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech.pytorch_amd.align import ForcedAligner  # noqa: E402
from deepspeech.pytorch_amd.configs import LABELS  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Word timings of reference transcripts on saved outputs (CTC forced alignment)")
    ap.add_argument("batches", nargs="+", help=".npz files with probs, sizes, targets, target_sizes")
    ap.add_argument("--output-path", default="align.json")
    ap.add_argument("--labels-path", default=None, help="JSON list of labels (default: the package's labels)")
    ap.add_argument("--frame-seconds", type=float, default=0.02, help="duration of one output frame")
    ap.add_argument("--min-mean-logp", type=float, default=None, help="flag clips whose score per frame is below this bar")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "align needs a HIP device"
    labels = LABELS
    if a.labels_path:
        with open(a.labels_path) as f:
            labels = json.load(f)
    aligner = ForcedAligner(labels, blank_index=labels.index('_') if '_' in labels else 0, frame_seconds=a.frame_seconds)
    alignments = []
    for path in a.batches:
        with np.load(path) as z:
            alignments += aligner.align(torch.from_numpy(z["probs"]).cuda(), torch.from_numpy(z["sizes"]),
                                        targets=torch.from_numpy(z["targets"]), target_sizes=torch.from_numpy(z["target_sizes"]),
                                        kind="probs")
    result = {"frame_seconds": a.frame_seconds,
              "clips": [{"score": al.score if al.feasible else None, "feasible": al.feasible, "frames": al.frames,
                         "words": [{"word": w.text, "start_frame": w.start_frame, "end_frame": w.end_frame, "start_s": w.start_s,
                                    "end_s": w.end_s, "logp": w.logp} for w in al.words]} for al in alignments]}
    if a.min_mean_logp is not None:
        result["flagged"] = ForcedAligner.flag(alignments, a.min_mean_logp)
    with open(a.output_path, "w") as f:
        json.dump(result, f, indent=1)
    print("%d clips aligned (%d infeasible) -> %s" % (len(alignments), sum(not al.feasible for al in alignments), a.output_path))


if __name__ == "__main__":
    main()
