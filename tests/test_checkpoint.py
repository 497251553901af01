"""Checkpoint interchange with the reference (gru4rec.py:742-781).

tests/golden/checkpoint/ref_checkpoint.pickle was written by the REFERENCE's own `savemodel` (oracle/make_checkpoint_fixture.py runs
the reference source on the Theano stand-in); ref_checkpoint_pred.npz holds what its `predict_next_batch` returned."""
import os
import pickle

import numpy as np
import pytest

from gru4rec_amd.gru4rec import GRU4Rec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'checkpoint')
PICKLE = os.path.join(GOLD, 'ref_checkpoint.pickle')
PRED = os.path.join(GOLD, 'ref_checkpoint_pred.npz')


def test_reference_pickle_loads_into_the_product_class():
    g = GRU4Rec.loadmodel(PICKLE)
    want = np.load(PRED, allow_pickle=False)
    assert isinstance(g, GRU4Rec)
    assert (g.loss, g.final_act, g.layers, g.embedding, g.constrained_embedding) == ('bpr-max', 'elu-0.5', [12], 8, False)
    np.testing.assert_array_equal(g.Wy, want['Wy'])
    np.testing.assert_array_equal(g.E, want['E'])
    np.testing.assert_array_equal(g.Wx[0], want['Wx0'])
    assert g.By.shape == (g.n_items, 1) and g.Wy.dtype == np.float32
    assert list(g.itemidmap.index.astype(str)) == list(want['itemids'])
    # the MI355X-side attributes the reference does not know get their defaults
    assert g.use_graph is True and g._model is None and g._loss_id is not None


def test_product_pickle_names_the_reference_class(tmp_path):
    """What the reference's loadmodel needs: module `gru4rec`, class `GRU4Rec`, NumPy arrays under the reference's
    attribute names, loss / activations as bound methods with the reference's method names."""
    g = GRU4Rec.loadmodel(PICKLE)
    f = str(tmp_path / 'm.pickle')
    g.savemodel(f)
    raw = open(f, 'rb').read()
    assert b'gru4rec_amd' not in raw and b'\x8c\x07gru4rec\x94\x8c\x07GRU4Rec' in raw
    h = GRU4Rec.loadmodel(f)
    st = h.__dict__
    for name in ('layers', 'loss', 'final_act', 'hidden_act', 'Wx', 'Wh', 'Wrz', 'Bh', 'H', 'Wy', 'By', 'E', 'itemidmap',
                 'n_items', 'loss_function', 'final_activation', 'hidden_activation', 'error_during_train'):
        assert name in st, name
    assert h.loss_function.__name__ == 'bpr_max' and h.hidden_activation.__name__ == 'tanh'
    assert type(h.final_activation.__self__).__name__ == 'Elu' and h.final_activation.__self__.alpha == 0.5
    assert '_model' not in pickle.loads(raw).__getstate__()
    np.testing.assert_array_equal(h.Wy, g.Wy)


class _ForeignReader(pickle.Unpickler):
    """Reads a checkpoint the way a process without this package does: `gru4rec.GRU4Rec` and the classes nested in it resolve to
    bare classes that only receive the pickled state, `getattr(obj, name)` -- how a bound method pickles -- to the name alone.
    Records what the file asks of its reader, for comparison with what the reference's environment resolved
    (tests/golden/checkpoint/ref_reader.npz, written by oracle/make_checkpoint_fixture.py with the reference's own loadmodel)."""
    def __init__(self, f):
        super().__init__(f)
        self.globals, self.getattrs = set(), set()

    def find_class(self, module, name):
        self.globals.add('%s %s' % (module, name))
        if module == 'gru4rec':
            return type(name.split('.')[-1], (), {})
        if (module, name) == ('builtins', 'getattr'):
            return lambda obj, attr, *default: self.getattrs.add(attr) or attr
        return super().find_class(module, name)


def _read_as_the_reference(path):
    """The state a reader without this package gets from `path`, after checking that the file asks no more of the reference's
    environment than it resolved when its own loadmodel read a product-written file."""
    with open(path, 'rb') as f:
        r = _ForeignReader(f)
        obj = r.load()
    rec = np.load(os.path.join(GOLD, 'ref_reader.npz'), allow_pickle=False)
    known = set(rec['globals'])
    assert {g for g in r.globals if g.startswith('gru4rec ')} <= known, 'names the reference module does not provide'
    assert r.getattrs <= set(rec['getattrs']), 'methods the reference class does not have'
    top = {g.split('.')[0].split(' ')[0] for g in known}
    assert {g.split('.')[0].split(' ')[0] for g in r.globals} <= top, 'modules the reference does not import'
    assert type(obj).__name__ == 'GRU4Rec'
    return obj.__dict__


def test_reference_reads_product_pickle(tmp_path):
    """A product-written pickle is what the reference's loadmodel + predict_next_batch read (gru4rec.py:665-781), without the
    reference: the file asks the reader for nothing the reference's environment did not resolve when the fixture generator
    loaded such a file with the reference's own loadmodel, and the reference's prediction -- restated by the NumPy oracle on the
    state as read -- reproduces the scores the reference gave (ref_checkpoint_pred.npz)."""
    from oracle.model import OracleGRU4Rec
    g = GRU4Rec.loadmodel(PICKLE)
    f = str(tmp_path / 'm.pickle')
    g.savemodel(f)
    st = _read_as_the_reference(f)
    want = np.load(PRED, allow_pickle=False)
    assert st['final_activation'] == 'execute' and st['loss_function'] == 'bpr_max' and st['hidden_activation'] == 'tanh'
    state = np.random.get_state()
    try:
        o = OracleGRU4Rec(n_items=st['n_items'], layers=st['layers'], batch_size=4, loss=st['loss'], final_act=st['final_act'],
                          hidden_act=st['hidden_act'], n_sample=0, constrained_embedding=st['constrained_embedding'],
                          embedding=st['embedding'])
    finally:
        np.random.set_state(state)
    o.E, o.Wy, o.By = st['E'], st['Wy'], np.asarray(st['By']).reshape(-1)
    o.Wx, o.Wh, o.Wrz, o.Bh = list(st['Wx']), list(st['Wh']), list(st['Wrz']), list(st['Bh'])
    ids = np.array(list(st['itemidmap'].index))
    in_idx = st['itemidmap'][ids[[0, 3, 5, 7]]].values
    yhat, _ = o.predict_step([np.zeros((4, D), dtype=np.float32) for D in st['layers']], in_idx)
    np.testing.assert_allclose(yhat.T, want['pred1'], rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
def test_reference_checkpoint_predicts_on_the_gpu():
    g = GRU4Rec.loadmodel(PICKLE)
    want = np.load(PRED, allow_pickle=False)
    ids = np.array(list(g.itemidmap.index))
    p1 = g.predict_next_batch(np.array([1, 2, 3, 4]), ids[[0, 3, 5, 7]], None, batch=4)
    p2 = g.predict_next_batch(np.array([1, 2, 9, 4]), ids[[2, 3, 1, 6]], None, batch=4)
    np.testing.assert_allclose(p1.values, want['pred1'], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(p2.values, want['pred2'], rtol=2e-4, atol=2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [dict(momentum=0.2, dropout_p_hidden=0.2, dropout_p_embed=0.1),
                                dict(adapt='adam', adapt_params=[0.9, 0.999], learning_rate=0.01, constrained_embedding=False, embedding=16),
                                dict(constrained_embedding=False, layers=[24]),
                                dict(train_random_order=True, momentum=0.1)],
                         ids=['adagrad_momentum_dropout', 'adam_separate_embedding', 'onehot', 'random_session_order'])
def test_resume_continues_bit_identically(tmp_path, kw):
    """SURVEY 8f rank 2, second half: 2 epochs == 1 epoch + savemodel(optimizer_state=True) + loadmodel + fit(resume=True).
    The sample store wraps around inside the epochs (its refill counter is part of the saved state), dropout masks are keyed by
    the global step."""
    from gru4rec_amd import synth
    data = synth.make_sessions(1500, n_items=300, seed=4)
    P = dict(loss='bpr-max', final_act='elu-0.5', layers=[32], batch_size=32, n_sample=64, constrained_embedding=True, learning_rate=0.1)
    P.update(kw)
    a = GRU4Rec(n_epochs=2, **P)
    a.fit(data.copy(), sample_store=64 * 50)
    b = GRU4Rec(n_epochs=1, **P)
    b.fit(data.copy(), sample_store=64 * 50)
    f = str(tmp_path / 'ckpt.pickle')
    b.savemodel(f, optimizer_state=True)
    b.close()
    c = GRU4Rec.loadmodel(f)
    assert c.epochs_done == 1 and c.optimizer_state['global_step'] == len(a.step_costs[0])
    c.n_epochs = 2
    c.fit(data.copy(), sample_store=64 * 50, resume=True)
    np.testing.assert_array_equal(c.step_costs[0], a.step_costs[1])
    np.testing.assert_array_equal(c.Wy, a.Wy)
    np.testing.assert_array_equal(c.By, a.By)
    for i in range(len(a.layers)):
        np.testing.assert_array_equal(c.Wx[i], a.Wx[i])
        np.testing.assert_array_equal(c.Wh[i], a.Wh[i])
    assert c.loss_history == a.loss_history
    if kw.get('train_random_order'):
        # the session order of the resumed epoch is the uninterrupted run's second permutation (NumPy's global stream travels in
        # the checkpoint), not a fresh draw
        assert not np.array_equal(a.step_costs[0], a.step_costs[1][:len(a.step_costs[0])])
    # a checkpoint without optimizer state refuses to resume instead of silently restarting the accumulators
    b2 = GRU4Rec.loadmodel(f)
    b2.optimizer_state = None
    with pytest.raises(ValueError):
        b2.fit(data.copy(), sample_store=64 * 50, resume=True)
    # ... and so does one whose optimizer state belongs to another configuration (the velocities would be dropped silently)
    b3 = GRU4Rec.loadmodel(f)
    b3.n_epochs = 2
    b3.momentum = 0.0 if b3.momentum > 0 else 0.3
    with pytest.raises(ValueError, match='momentum'):
        b3.fit(data.copy(), sample_store=64 * 50, resume=True)
    # the host sampler cannot resume, and says so before anything is built
    b4 = GRU4Rec.loadmodel(f)
    b4.n_epochs = 2
    with pytest.raises(NotImplementedError):
        b4.fit(data.copy(), sample_store=64 * 50, store_type='cpu', resume=True)
    assert b4._model is None


def test_checkpoint_with_optimizer_state_keeps_the_reference_layout(tmp_path):
    """The extra attributes ride along; everything the reference's loadmodel reads is unchanged."""
    g = GRU4Rec.loadmodel(PICKLE)
    g.optimizer_state = {'arrays': {('acc_Wy', 0): np.ones((g.n_items, 12), dtype=np.float32)}, 'global_step': 7, 'refills': 1}
    g.epochs_done = 3
    f = str(tmp_path / 'm.pickle')
    with open(f, 'wb') as fh:
        pickle.dump(g, fh)
    h = GRU4Rec.loadmodel(f)
    assert h.epochs_done == 3 and h.optimizer_state['global_step'] == 7
    np.testing.assert_array_equal(h.Wy, g.Wy)
    back = _read_as_the_reference(f)      # what the reference's loader resolves is all the file asks for
    assert back['epochs_done'] == 3
    np.testing.assert_array_equal(back['Wy'], g.Wy)
