"""Decodes saved network outputs into words with timings and confidences (decode_words of the device CTC decoders).

    python tools/decode_words.py --output-path words.json [--beam-width 100 --lm-path lm.arpa --alpha 1.2 --beta 0.8]
                                 [--hotwords "NEW YORK" ...] [--measure entropy --aggregate mean --word-aggregate min] batch0.npz ...

Each .npz holds one batch, the same files tools/align.py and tools/search_lm_params.py read: probs (N, T', C) probabilities and
sizes (N) valid frames (targets are ignored).  --beam-width 0 decodes greedily.  The JSON holds, per clip in the order of the
files, the transcript, its confidence (null without words), with a beam search score and acoustic, and the words as {word,
start_frame, end_frame, start_s, end_s, confidence}.  The confidence measures are defined in DESIGN.md section 3.8; they are
not calibrated on any data.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepspeech.pytorch_amd.confidence import AGGREGATES, MEASURES, Confidence  # noqa: E402
from deepspeech.pytorch_amd.configs import LABELS  # noqa: E402
from deepspeech.pytorch_amd.decoder import BeamCTCDecoder, GreedyDecoder  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Words with timings and confidences from saved outputs")
    ap.add_argument("batches", nargs="+", help=".npz files with probs and sizes")
    ap.add_argument("--output-path", default="words.json")
    ap.add_argument("--labels-path", default=None, help="JSON list of labels (default: the package's labels)")
    ap.add_argument("--frame-seconds", type=float, default=0.02, help="duration of one output frame")
    ap.add_argument("--beam-width", type=int, default=100, help="0: greedy decoding")
    ap.add_argument("--lm-path", default=None, help="ARPA file of a word n-gram model")
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--cutoff-top-n", type=int, default=40)
    ap.add_argument("--cutoff-prob", type=float, default=1.0)
    ap.add_argument("--hotwords", nargs="*", default=None, help="phrases the search should prefer")
    ap.add_argument("--hotword-weight", type=float, default=2.0)
    ap.add_argument("--measure", default="label_prob", choices=sorted(MEASURES))
    ap.add_argument("--entropy-alpha", type=float, default=1 / 3, help="order of the tsallis / renyi entropy")
    ap.add_argument("--aggregate", default="mean", choices=sorted(AGGREGATES))
    ap.add_argument("--word-aggregate", default="min", choices=sorted(AGGREGATES))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "decode_words needs a HIP device"
    labels = LABELS
    if a.labels_path:
        with open(a.labels_path) as f:
            labels = json.load(f)
    blank = labels.index('_') if '_' in labels else 0
    conf = Confidence(a.measure, a.entropy_alpha, a.aggregate, a.word_aggregate)
    if a.beam_width > 0:
        dec = BeamCTCDecoder(labels, lm_path=a.lm_path, alpha=a.alpha, beta=a.beta, cutoff_top_n=a.cutoff_top_n,
                             cutoff_prob=a.cutoff_prob, beam_width=a.beam_width, blank_index=blank, hotwords=a.hotwords,
                             hotword_weight=a.hotword_weight)
    else:
        dec = GreedyDecoder(labels, blank_index=blank)
    hyps = []
    for path in a.batches:
        with np.load(path) as z:
            probs, sizes = torch.from_numpy(z["probs"]).cuda(), torch.from_numpy(z["sizes"])
        out = dec.decode_words(probs, sizes, confidence=conf, frame_seconds=a.frame_seconds)
        hyps += [o[0] for o in out] if a.beam_width > 0 else out
    result = {"frame_seconds": a.frame_seconds, "confidence": repr(conf),
              "clips": [{"transcript": h.text, "confidence": h.confidence, "score": h.score, "acoustic": h.acoustic,
                         "words": [{"word": w.text, "start_frame": w.start_frame, "end_frame": w.end_frame, "start_s": w.start_s,
                                    "end_s": w.end_s, "confidence": w.confidence} for w in h.words]} for h in hyps]}
    with open(a.output_path, "w") as f:
        json.dump(result, f, indent=1)
    print("%d clips, %d words -> %s" % (len(hyps), sum(len(h.words) for h in hyps), a.output_path))


if __name__ == "__main__":
    main()
