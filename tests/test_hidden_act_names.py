"""The hidden activation's names and its reference derivative (no GPU).

The product (gru4rec_amd.gru4rec._parse_act) and the oracle (oracle.model.parse_act) each turn 'selu-<lambda>-<alpha>' & co. into
(kind, p0, p1); tests/test_gpu_hidden_act.py hands the oracle's triple to the library and compares against the oracle, so the two
parsers have to agree -- the order of selu's two numbers included.  oracle.model.act_bwd, the derivative every GPU parity test of
the backward kernels leans on, is pinned here against a central finite difference of act_fwd in float64."""
import numpy as np
import pytest

from gru4rec_amd import _native
from gru4rec_amd.gru4rec import GRU4Rec, _parse_act
from oracle.model import act_bwd, act_fwd, parse_act

HIDDEN_ACTS = ['tanh', 'relu', 'linear', 'leaky-0.2', 'elu-0.5', 'selu-1.0507-1.6733']


@pytest.mark.parametrize('name', HIDDEN_ACTS)
def test_product_and_oracle_parse_the_same_triple(name):
    kind, p0, p1 = parse_act(name)
    assert _parse_act(name, False) == (_native.ACT_IDS[kind], p0, p1)


def test_selu_parameter_order():
    """'selu-<lambda>-<alpha>' (the reference's Selu(lmbd, alpha)): p0 is the outer scale, p1 the factor of exp(x) - 1."""
    assert parse_act('selu-1.0507-1.6733') == ('selu', 1.0507, 1.6733)
    assert _parse_act('selu-1.0507-1.6733', False) == (_native.ACT_IDS['selu'], 1.0507, 1.6733)
    x = np.array([2.0, -30.0])
    np.testing.assert_allclose(act_fwd('selu', 1.0507, 1.6733, x), [2.0 * 1.0507, -1.0507 * 1.6733], rtol=1e-12)


@pytest.mark.parametrize('name', ['softmax', 'softmax_logit'])
def test_softmax_names_are_no_hidden_activations(name):
    with pytest.raises(NotImplementedError):
        _parse_act(name, False)
    with pytest.raises(NotImplementedError):
        GRU4Rec(hidden_act=name)
    _parse_act(name, True)      # (both are final activations)


@pytest.mark.parametrize('name', HIDDEN_ACTS)
def test_oracle_derivative_is_the_finite_difference_of_its_forward(name):
    """float64, |x| in [0.05, 3] on both sides of the kink, central difference with h = 1e-6: truncation h^2 |f'''| / 6 < 1e-12,
    rounding eps64 |f| / h < 1e-9 -- bound 1e-8."""
    kind, p0, p1 = parse_act(name)
    mag = np.linspace(0.05, 3.0, 60)
    x = np.concatenate([-mag[::-1], mag])
    h = 1e-6
    fd = (act_fwd(kind, p0, p1, x + h) - act_fwd(kind, p0, p1, x - h)) / (2 * h)
    got = act_bwd(kind, p0, p1, x, act_fwd(kind, p0, p1, x))
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, fd, rtol=0, atol=1e-8)
    if kind in ('leaky', 'elu', 'selu'):      # the two slopes at the kink: 1 | alpha (leaky, elu), lambda | lambda alpha (selu)
        edge = act_bwd(kind, p0, p1, np.array([1e-9, -1e-9]), act_fwd(kind, p0, p1, np.array([1e-9, -1e-9])))
        want = {'leaky': (1.0, p0), 'elu': (1.0, p0), 'selu': (p0, p0 * p1)}[kind]
        np.testing.assert_allclose(edge, want, rtol=1e-8)
