"""What the byte-exact suites (test_relation_bits_gpu.py, test_score_bits_gpu.py) share: inputs from integer arithmetic alone,
identical on any machine and library version, one SHA-256 per case over the output tensors' bytes, and the recorder

    python tests/test_<family>_bits_gpu.py --record [--out PATH] [--commit ID]

which writes the fixture (on the MI355X, at the build whose bits are to be kept)."""

import hashlib
import json
import os

import numpy as np
import torch


def hashed(n, m, salt):
    """fp32 [n, m] in [-0.5, 0.5): 16 bits of a multiplicative hash of (i, j, salt)."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(m, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(salt) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h = ((h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    return ((h.astype(np.int64) - 32768).astype(np.float32) / np.float32(65536.0))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def affine(n, mul, add, mod):
    return dev((np.arange(n, dtype=np.int64) * mul + add) % mod)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def load_fixture(path):
    with open(path) as f:
        return json.load(f)["cases"]


def record_main(fixture, cases):
    """The command line of a bits suite: run every case and write its digest to the fixture."""
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true", required=True)
    ap.add_argument("--out", default=fixture)
    ap.add_argument("--commit", default=None, help="the commit whose build is recorded")
    args = ap.parse_args()
    doc = {"recorded_at": args.commit, "device": torch.cuda.get_device_name(0),
           "cases": {name: digest(cases[name]()) for name in sorted(cases)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(doc['cases'])} cases to {args.out}")
