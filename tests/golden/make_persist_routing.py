"""Records the routing table of the persistent recurrent sweeps into tests/golden/routing/persist_routing.npz (a directory of its own:
every tests/golden/*.npz is a model fixture).

    python tests/golden/make_persist_routing.py --commit <hash of the commit the library was built from> [--lib libds2hip.so] [--out x.npz]

Run on an MI355X (256 CUs) with the library of the commit whose routing is to be pinned -- never with the code under test.
For every problem of the grid it asks the live entries ds2_rnn_persist_supported / _kind / _ws_bytes under each `variant`
and ds2_rnn_persist_shape_covered, and stores the answers as integer arrays indexed [cell][D - 1][H index][N index][variant index]:

    H, N, variants                  the grid axes (cells are 0 GRU, 1 LSTM, 2 RNN; D is 1, 2)
    bf16_supported / _kind / _ws    bf16 rows under every variant of `variants`
    f32_supported / _kind / _ws     fp32 rows under variants[:2] (no bit changes an fp32 answer; the two columns being equal shows it)
    bf16_covered, f32_covered       ds2_rnn_persist_shape_covered, [cell][D - 1][H index][N index]
    header                          utf-8 bytes: which commit and device wrote the table

tests/test_host.py checks the plan against it with 256 CUs given explicitly; tests/test_gpu_kernels.py checks the live entries.
"""
import argparse
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32, BF16 = 0, 1
HS = list(range(16, 1601, 16))
NS = list(range(1, 73)) + [80, 81, 96, 97, 128, 129, 160, 161, 256, 257, 320, 321, 512, 513, 1024, 1025, 2048, 2049]
VARIANTS = [0, 1, 2, 8, 16, 32, 64, 128]


def record(lib, dtype, variants):
    shape = (3, 2, len(HS), len(NS))
    sup = np.zeros(shape + (len(variants),), np.int8)
    kind = np.zeros(shape + (len(variants),), np.int8)
    ws = np.zeros(shape + (len(variants),), np.int64)
    cov = np.zeros(shape, np.int8)
    for cell in range(3):
        for D in (1, 2):
            for hi, H in enumerate(HS):
                for ni, N in enumerate(NS):
                    cov[cell, D - 1, hi, ni] = lib.ds2_rnn_persist_shape_covered(dtype, cell, D, N, H)
                    for vi, v in enumerate(variants):
                        sup[cell, D - 1, hi, ni, vi] = lib.ds2_rnn_persist_supported(dtype, cell, D, N, H, v)
                        kind[cell, D - 1, hi, ni, vi] = lib.ds2_rnn_persist_kind(dtype, cell, D, N, H, v)
                        ws[cell, D - 1, hi, ni, vi] = lib.ds2_rnn_persist_ws_bytes(dtype, cell, D, N, H, v)
    return sup, kind, ws, cov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--lib", default=os.path.join(HERE, "..", "..", "deepspeech", "pytorch_amd", "libds2hip.so"))
    ap.add_argument("--out", default=os.path.join(HERE, "routing", "persist_routing.npz"))
    a = ap.parse_args()
    lib = C.CDLL(os.path.abspath(a.lib))
    q = [C.c_int] * 5
    for name, res, args in (("supported", C.c_int, q + [C.c_uint]), ("kind", C.c_int, q + [C.c_uint]),
                            ("ws_bytes", C.c_long, q + [C.c_uint]), ("shape_covered", C.c_int, q)):
        fn = getattr(lib, "ds2_rnn_persist_" + name)
        fn.restype, fn.argtypes = res, args
    bs, bk, bw, bc = record(lib, BF16, VARIANTS)
    fs, fk, fw, fc = record(lib, F32, VARIANTS[:2])
    live = bool(bk.any())     # a device below 256 CUs answers 0 everywhere
    header = "persistent-sweep routing table recorded from commit %s on a device that %s" % (
        a.commit, "runs the persistent sweeps (>= 256 CUs)" if live else "does NOT run them (only the *_covered arrays mean anything)")
    np.savez_compressed(a.out, H=np.array(HS, np.int32), N=np.array(NS, np.int32), variants=np.array(VARIANTS, np.int32),
                        bf16_supported=bs, bf16_kind=bk, bf16_ws=bw, bf16_covered=bc,
                        f32_supported=fs, f32_kind=fk, f32_ws=fw, f32_covered=fc,
                        header=np.frombuffer(header.encode(), np.uint8))
    print(header)
    print("rows: bf16 %d x %d variants, fp32 %d x 2; kinds seen: %s; %d bytes" % (
        bc.size, len(VARIANTS), fc.size, sorted(set(np.unique(bk)) | set(np.unique(fk))), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
