#!/usr/bin/env python
"""Checkpoint interchange fixture (gru4rec.py:742-781).  TEST INFRASTRUCTURE.

1. The REFERENCE's own source (on the Theano stand-in) trains a small model and writes it with its own `savemodel`
   -> tests/golden/checkpoint/ref_checkpoint.pickle, plus the scores its `predict_next_batch` gives for two batches
   -> tests/golden/checkpoint/ref_checkpoint_pred.npz.
2. Reverse direction, checked here because it needs the reference source: the product class loads that pickle, writes it
   again with ITS `savemodel`, and the reference's `loadmodel` + `predict_next_batch` must reproduce the same scores.  What the
   reference's environment resolved while reading the product-written files -- every global, and every attribute a `getattr` in
   the pickle asked of the reference's objects (bound methods pickle that way) -- is recorded in
   tests/golden/checkpoint/ref_reader.npz: tests/test_checkpoint.py holds today's product-written files to it.
Run:  python oracle/make_checkpoint_fixture.py
"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle import make_golden  # noqa: E402  (data generator, RNG hook)

OUT = os.path.join(ROOT, 'tests', 'golden', 'checkpoint')
PARAMS = dict(loss='bpr-max', final_act='elu-0.5', hidden_act='tanh', layers=[12], n_epochs=1, batch_size=8,
              dropout_p_embed=0.0, dropout_p_hidden=0.0, learning_rate=0.1, momentum=0.0, n_sample=16, sample_alpha=0.5,
              bpreg=1.0, constrained_embedding=False, embedding=8)


def predictions(gru, ids):
    p1 = gru.predict_next_batch(np.array([1, 2, 3, 4]), ids[[0, 3, 5, 7]], None, batch=4)
    p2 = gru.predict_next_batch(np.array([1, 2, 9, 4]), ids[[2, 3, 1, 6]], None, batch=4)
    return p1.values.astype(np.float32), p2.values.astype(np.float32)


def reader_record(paths):
    """(globals as 'module name', getattr attribute names) the reference's environment resolves reading the pickles `paths`:
    the reference's `gru4rec` module must be loaded under that name (ref_loader.load)."""
    seen, attrs = set(), set()

    def rec_getattr(obj, name, *default):
        attrs.add(name)
        return getattr(obj, name, *default)

    class Recorder(pickle.Unpickler):
        def find_class(self, module, name):
            seen.add('%s %s' % (module, name))
            if (module, name) == ('builtins', 'getattr'):
                return rec_getattr
            return super().find_class(module, name)
    for p in paths:
        with open(p, 'rb') as f:
            Recorder(f).load()
    return sorted(seen), sorted(attrs)


def main():
    theano, ref, _ = ref_loader.load()
    theano._rng_nodes.clear()
    theano.CALL_LOG.clear()
    data = make_golden.make_data(7)
    train = data[data.SessionId <= 55].copy()
    make_golden.install_rng_hook(PARAMS, {'refills': 0})
    gru = ref.GRU4Rec(**PARAMS)
    gru.fit(train.copy(), sample_store=make_golden.SAMPLE_STORE_ROWS * PARAMS['n_sample'], store_type='gpu')
    ids = np.array(list(gru.itemidmap.index))
    p1, p2 = predictions(gru, ids)
    path = os.path.join(OUT, 'ref_checkpoint.pickle')
    gru.savemodel(path)                                       # the reference's own writer
    np.savez_compressed(os.path.join(OUT, 'ref_checkpoint_pred.npz'), pred1=p1, pred2=p2, itemids=ids.astype(str),
                        Wy=gru.Wy.get_value(), E=gru.E.get_value(), Wx0=gru.Wx[0].get_value(), params=str(PARAMS))
    # ---- reverse direction: product writes, reference reads
    ref_loader.unload()
    from gru4rec_amd.gru4rec import GRU4Rec
    sys.modules['gru4rec'] = sys.modules['gru4rec_amd.gru4rec']
    mine = GRU4Rec.loadmodel(path)
    tmp = os.path.join(tempfile.mkdtemp(prefix='g4r_ckpt_'), 'product_checkpoint.pickle')
    mine.savemodel(tmp)                                       # the product's writer
    tmp_opt = tmp + '.opt'                                    # ... and a file with the optimizer-state extras (test_checkpoint.py)
    mine.optimizer_state = {'arrays': {('acc_Wy', 0): np.ones((mine.n_items, 12), dtype=np.float32)}, 'global_step': 7, 'refills': 1}
    mine.epochs_done = 3
    with open(tmp_opt, 'wb') as fh:
        pickle.dump(mine, fh)
    _, ref2, _ = ref_loader.load()
    back = ref2.GRU4Rec.loadmodel(tmp)                        # the reference's own reader
    q1, q2 = predictions(back, ids)
    np.testing.assert_array_equal(q1, p1)
    np.testing.assert_array_equal(q2, p2)
    assert ref2.GRU4Rec.loadmodel(tmp_opt).epochs_done == 3
    seen, attrs = reader_record([tmp, tmp_opt])
    np.savez_compressed(os.path.join(OUT, 'ref_reader.npz'), globals=np.array(seen), getattrs=np.array(attrs))
    print('reference -> product -> reference round trip reproduces the reference predictions bit for bit')
    print('the reference resolved %d globals and %d attributes reading the product\'s files' % (len(seen), len(attrs)))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
