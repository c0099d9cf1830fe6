"""Writes tests/golden/l3ic_streams.npz: seeded index layers and the layer payloads tests/l3ic_ref.py codes them to (RLE,
RAW and rANS at lane counts 1, 2 and 16).  It pins the l3ic payload format against later drift.
    python tests/golden/make_l3ic_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import l3ic_ref  # noqa: E402


def laplace_layer(rng, n, k, scale):
    p = np.exp(-np.abs(np.arange(k) - (k - 1) / 2) / scale)
    return rng.choice(k, n, p=p / p.sum()).astype(np.uint8)


def main():
    rng = np.random.default_rng(20261016)
    layers = [                                  # (indices, codebook size)
        (laplace_layer(rng, 4096, 32, 2.0), 32),            # rANS, 2 lanes
        (laplace_layer(rng, 1000, 256, 1.5), 256),          # rANS, 1 lane, 2-byte frequencies
        (laplace_layer(rng, 65025, 4, 0.3), 4),             # rANS, 16 lanes
        (rng.integers(0, 256, 300).astype(np.uint8), 256),  # RAW
        (np.full(64, 9, np.uint8), 32),                     # RLE
        (np.array([0, 1, 1, 0, 1], np.uint8), 2),           # RAW (rANS would not be shorter)
    ]
    out = {}
    for i, (sym, k) in enumerate(layers):
        out['sym{}'.format(i)] = sym
        out['k{}'.format(i)] = np.int32(k)
        out['payload{}'.format(i)] = np.frombuffer(l3ic_ref.encode_layer(sym, k), np.uint8)
    path = os.path.join(HERE, 'l3ic_streams.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', [len(out['payload{}'.format(i)]) for i in range(len(layers))])


if __name__ == '__main__':
    main()
