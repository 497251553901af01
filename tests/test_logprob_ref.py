"""The host twin of sample_sessions' log-probabilities and nucleus (tests/logprob_ref.py) on fixed arrays, without a GPU."""
import numpy as np

import logprob_ref as lref


def terms64(z, zeta, inv_t):
    """The terms from the float64 twin, rounded to integers (the device's come from expf)."""
    return np.rint(lref.q64(lref.d32(z, zeta, inv_t))).astype(np.uint64)


def test_terms_and_sums():
    z = np.array([2.0, 1.0, 2.0, -40.0, np.nan], dtype=np.float32)
    d = lref.d32(z, 2.0, 0.5)
    assert d.dtype == np.float32 and d[:4].tolist() == [0.0, -0.5, 0.0, -21.0] and np.isnan(d[4])
    q = lref.q64(d)
    assert q[0] == q[2] == 2.0 ** 39 and q[4] == 0.0 and abs(q[1] - 2.0 ** 39 * np.exp(-0.5)) < 1e-3
    assert lref.q64(np.float32(-28.0)) < 0.5                      # about 27 nats below zeta a term rounds to 0
    assert lref.total(np.array([2 ** 62, 2 ** 62 - 1, 1], dtype=np.uint64)) == 2 ** 63       # exact where float64 is not
    # two roundings: fl32(z - zeta) first
    zz, zeta = np.float32(1e-8), np.float32(1.0)
    assert lref.d32(zz, zeta, 3.0) == np.float32(np.float32(zz - zeta) * np.float32(3.0))
    Q = 3 * 2 ** 39
    assert lref.lse(2.0, 0.5, Q) == np.float32(1.0 + np.log(3.0))
    assert lref.logprob(0.0, 2 ** 39) == 0.0 and lref.logprob(-0.5, Q) == np.float32(-0.5 - np.log(3.0))


def test_the_nucleus_rule():
    q = [2 ** 39, 2 ** 38, 2 ** 38, 2 ** 37]
    Q = sum(q) + 2 ** 37                                            # the eligible set holds more than the t best
    assert lref.nucleus(q, 1.0, sum(q)) == (4, sum(q))              # top_p = 1 over the t best alone keeps all
    assert lref.nucleus(q, 1e-6, Q) == (1, 2 ** 39)                 # a tiny top_p keeps one
    assert lref.nucleus(q, 1.0, Q) == (4, sum(q))                   # no prefix reaches the mass: m = t
    assert lref.nucleus(q, 0.5, Q) == (2, 2 ** 39 + 2 ** 38)        # 4 / 10 < 0.5 <= 6 / 10
    share = np.float32(0.4)                                 # the first entry's share, to a float32 ulp
    assert lref.nucleus(q, np.nextafter(share, np.float32(1)), Q)[0] == 2
    assert lref.nucleus(q, np.nextafter(share, np.float32(0)), Q)[0] == 1
    # the threshold is float64(fl32(top_p)) * float64(Q), not the float64 top_p
    assert lref.nucleus([1, 1], 0.1, 10) == (2, 2) and np.float64(np.float32(0.1)) * 10 > 1.0
    assert lref.nucleus([1, 1], 0.099999, 10) == (1, 1)


def test_draws_take_equal_z_in_selection_order():
    z = np.array([1.0, 3.0, 3.0, 3.0, 0.0], dtype=np.float32)
    on = np.ones(5, dtype=bool)
    g0 = np.zeros(5, dtype=np.float32)
    # top_k = 2 of three equal z: positions 1 and 2; noise on position 3 cannot bring it in, noise on 2 wins
    g = np.array([0, 0, 1, 9, 0], dtype=np.float32)
    p, lp, zeta, Q = lref.draw(z, g, 1.0, on, terms64, top_k=2)
    assert (p, zeta, Q) == (2, 3.0, None) and lp == np.float32(-np.log(2.0))
    # top_p = 0.3 of the whole mass (3 + e^-2 + e^-3) 2^39: the first entry's share is above it
    p, lp, zeta, Q = lref.draw(z, g, 1.0, on, terms64, top_k=3, top_p=0.3)
    assert p == 1 and lp == 0.0 and Q == lref.total(terms64(z, 3.0, 1.0))
    p, lp, _, _ = lref.draw(z, g, 1.0, on, terms64, top_k=3, top_p=0.5)
    assert p == 2 and lp == np.float32(-np.log(2.0))
    # top_p = 1: the three equal entries do not reach the whole mass, so m = t and top_p=None's draw
    assert lref.draw(z, g, 1.0, on, terms64, top_k=3, top_p=1.0)[:2] == lref.draw(z, g, 1.0, on, terms64, top_k=3)[:2]
    # untruncated: Den = Q, ineligible positions neither drawn nor counted
    off = on.copy()
    off[1] = False
    p, lp, zeta, Q = lref.draw(z, g0, 1.0, off, terms64)
    assert p == 2 and Q == lref.total(terms64(z, 3.0, 1.0)[off]) and lp == lref.logprob(0.0, Q)
    # a temperature: d is scaled after the subtraction
    p, lp, zeta, Q = lref.draw(z, g0, 0.5, on, terms64, top_k=5)
    assert lp == lref.logprob(0.0, lref.total(terms64(z, 3.0, 0.5)))
