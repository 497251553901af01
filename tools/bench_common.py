"""The serving model of the tools/bench_*.py tools: a device model with random weights (no fit: only the serving path is timed)."""
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gru4rec_amd import _native  # noqa: E402
from gru4rec_amd.gru4rec import GRU4Rec  # noqa: E402


def tiled_weights(I, D, rng, blk=4093, by=0.1, w=0.05):
    """The six parameters in upload order from a np.random.RandomState; Wy is one random block of blk rows, repeated."""
    yield 'Wy', np.tile((rng.randn(blk, D) * 0.1).astype(np.float32), (I // blk + 1, 1))[:I]
    yield 'By', (rng.randn(I) * by).astype(np.float32)
    yield 'Wx', (rng.randn(D, 3 * D) * w).astype(np.float32)
    yield 'Wh', (rng.randn(D, D) * w).astype(np.float32)
    yield 'Wrz', (rng.randn(D, 2 * D) * w).astype(np.float32)
    yield 'Bh', (rng.randn(3 * D) * 0.1).astype(np.float32)


def dense_weights(I, D, rng):
    """The same from a np.random.Generator, every row of Wy drawn (the bf16 scan and the neighbour search depend on the rows)."""
    Wy = np.empty((I, D), dtype=np.float32)
    for b in range(0, I, 1 << 20):      # (in blocks: no float64 copy of the whole table)
        Wy[b:b + (1 << 20)] = rng.standard_normal((min(1 << 20, I - b), D), dtype=np.float32) * np.float32(0.1)
    yield 'Wy', Wy
    del Wy
    yield 'By', (rng.standard_normal(I, dtype=np.float32) * np.float32(0.05))
    yield 'Wx', (rng.standard_normal((D, 3 * D)) * 0.05).astype(np.float32)
    yield 'Wh', (rng.standard_normal((D, D)) * 0.05).astype(np.float32)
    yield 'Wrz', (rng.standard_normal((D, 2 * D)) * 0.05).astype(np.float32)
    yield 'Bh', (rng.standard_normal(3 * D) * 0.1).astype(np.float32)


def serving_model(I, D, rows, act, rng, weights=tiled_weights, seed=1, keep=None):
    """_native.Model of I items x D units for batches of `rows`, final activation act, its parameters drawn from rng by `weights`.
    keep: a dict; the parameters it names are stored in it."""
    sm = act.startswith('softmax')
    m = _native.Model(n_items=I, layers=[D], batch_size=rows, n_sample=0, loss=_native.LOSS_IDS['cross-entropy' if sm else 'bpr-max'],
                      final_act=_native.ACT_IDS[act], hidden_act=_native.ACT_IDS['tanh'], embed_mode=0, embedding=0, learning_rate=0.1,
                      sample_store=0, seed=seed, device=0, rank=0, nranks=1, use_graph=0)
    for name, a in weights(I, D, rng):
        m.set_param(name, a)
        if keep is not None and name in keep:
            keep[name] = a
    return m


def as_gru4rec(m, I, D, act):
    """A bare GRU4Rec around the device model m: item ids 1000 ..., no fit."""
    g = GRU4Rec(layers=[D], final_act=act, loss='bpr-max')
    g.itemidmap = pd.Series(data=np.arange(I), index=np.arange(I) + 1000, name='ItemIdx')
    g.n_items = I
    g.error_during_train = False
    g._model = m
    return g
