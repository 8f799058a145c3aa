"""Grid search of the language-model weights alpha and beta of BeamCTCDecoder on saved network outputs: the device counterpart of
the reference's search_lm_params.py.  Every batch is decoded at all grid points in one launch and its errors are counted on the
device (deepspeech.pytorch_amd.lm_search.LMGridSearch); the result is the JSON list of [alpha, beta, WER, CER] that the
reference's select_lm_params.py reads.

    python tools/search_lm_params.py --lm-path lm.arpa --output-path search.json batch0.npz batch1.npz ...

Each .npz holds one batch of the model's outputs: probs (N, T', C) probabilities, sizes (N) valid frames, targets (the references'
labels back to back) and target_sizes (N).  Producing them (the model forward and the data loader) stays with the user.
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
from deepspeech.pytorch_amd.decoder import BeamCTCDecoder  # noqa: E402
from deepspeech.pytorch_amd.lm_search import LMGridSearch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Search alpha and beta of the n-gram LM decoder on saved outputs")
    ap.add_argument("batches", nargs="+", help=".npz files with probs, sizes, targets, target_sizes")
    ap.add_argument("--lm-path", required=True, help="ARPA text file of the n-gram model")
    ap.add_argument("--output-path", default="lm_search.json")
    ap.add_argument("--labels-path", default=None, help="JSON list of labels (default: the package's labels)")
    ap.add_argument("--alpha-from", type=float, default=0.0)
    ap.add_argument("--alpha-to", type=float, default=3.0)
    ap.add_argument("--beta-from", type=float, default=0.0)
    ap.add_argument("--beta-to", type=float, default=1.0)
    ap.add_argument("--num-alphas", type=int, default=25)
    ap.add_argument("--num-betas", type=int, default=20, help="num-alphas x num-betas points (the reference runs 500 trials)")
    ap.add_argument("--beam-width", type=int, default=10)
    ap.add_argument("--cutoff-top-n", type=int, default=40)
    ap.add_argument("--cutoff-prob", type=float, default=1.0)
    ap.add_argument("--open-vocabulary", action="store_true", help="lexicon=False: words outside the LM's vocabulary survive")
    ap.add_argument("--lm-unit", default="word", choices=["word", "char", "auto"],
                    help="what the model's units are: words, characters (every label is an event), or by ctcdecode's test")
    ap.add_argument("--space-token", default=None, help="character mode: the unigram that stands for the space label, e.g. '|'")
    ap.add_argument("--max-ws-mb", type=int, default=1024, help="workspace cap of one launch; larger grids run in chunks")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "search_lm_params needs a HIP device"
    labels = LABELS
    if a.labels_path:
        with open(a.labels_path) as f:
            labels = json.load(f)
    dec = BeamCTCDecoder(labels, a.lm_path, cutoff_top_n=a.cutoff_top_n, cutoff_prob=a.cutoff_prob, beam_width=a.beam_width,
                         blank_index=labels.index('_') if '_' in labels else 0, lexicon=not a.open_vocabulary, lm_unit=a.lm_unit,
                         space_token=a.space_token)
    search = LMGridSearch.from_ranges(a.alpha_from, a.alpha_to, a.num_alphas, a.beta_from, a.beta_to, a.num_betas, decoder=dec,
                                      max_ws_bytes=a.max_ws_mb << 20)
    for path in a.batches:
        with np.load(path) as z:
            search.update(torch.from_numpy(z["probs"]).cuda(), torch.from_numpy(z["sizes"]), torch.from_numpy(z["targets"]),
                          torch.from_numpy(z["target_sizes"]))
    search.save(a.output_path)
    print("Alpha: %f \nBeta: %f \nWER: %f\nCER: %f" % tuple(search.best()))
    print("%d points written to %s" % (len(search.points), a.output_path))


if __name__ == "__main__":
    main()
