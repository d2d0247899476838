"""Systems whose oscillators and pairs all differ, and the partial collapse types, on the CPU: the inputs of tests/test_gpu_unequal_constants.py
and the oracle they are compared with.

helpers.unequal_constants gives every oscillator its own self-Kerr, T1 and T2 and every pair its own cross-Kerr and J (one oscillator
without decay from three oscillators on).  Here the oracle's operator on such systems is held against the master equation written with
Kronecker products (helpers.master_equation_rhs, independent of the oracle and of every golden file), under collapse_type decay, dephase
and both.  The same tests state what makes the fixture worth running: exchanging the constants of two pairs or of two oscillators moves
the Kronecker result by at least 1e-6 of its maximum - seven orders above the 1e-13 the operators are compared at - so a kernel that read
a constant with the wrong index could not pass."""
import numpy as np
import pytest

from helpers import master_equation_rhs, synthetic_cfg, synthetic_spec, unequal_constants
from oracle.oracle import Oracle
from quandary_amd import capi, config

WITNESS = 1e-6  # of max |M x|: the least an exchanged pair of constants must move the operator


def test_default_config_text_is_unchanged():
    """The keywords for unequal constants default to the lines synthetic_cfg always wrote: every other test sees the system it saw."""
    text = synthetic_cfg([2, 2])
    for line in ("selfkerr = 0.2,0.2", "crosskerr = 0.001", "Jkl = 0.0", "collapse_type = both", "decay_time = 80.0,80.0", "dephase_time = 26.0,26.0"):
        assert line in text.split("\n"), line
    assert "collapse_type = none" in synthetic_cfg([2, 2], lindblad=False).split("\n")
    assert "Jkl = 0.02" in synthetic_cfg([3, 2, 2], jkl=0.02).split("\n")
    assert "selfkerr = 0.2,0.2,0.2" in synthetic_cfg([3, 2, 2]).split("\n")


@pytest.mark.parametrize("Q", [2, 3, 4, 5, 6])
def test_unequal_constants_are_all_distinct(Q):
    for zero_pair in (None, 1 if Q > 2 else 0):
        kw = unequal_constants(Q, zero_pair=zero_pair)
        npairs = Q * (Q - 1) // 2
        for key, n in (("selfkerr", Q), ("decay_time", Q), ("dephase_time", Q), ("crosskerr", npairs), ("jkl_pairs", npairs)):
            assert len(kw[key]) == n and len(set(kw[key])) == n, key
        assert (min(kw["decay_time"]) == 0.0) == (Q >= 3) and min(kw["dephase_time"]) > 0
        assert (min(kw["jkl_pairs"]) == 0.0) == (zero_pair is not None)
    assert "jkl_pairs" not in unequal_constants(Q, coupled=False)
    sp = synthetic_spec([2] * Q, **unequal_constants(Q))
    assert list(sp.system.crosskerr[:npairs]) == kw["crosskerr"] and list(sp.system.selfkerr[:Q]) == kw["selfkerr"]


def test_build_spec_short_vectors_and_collapse_types():
    """src/config.cpp copyLast: a vector shorter than the number of oscillators or pairs repeats its last entry; collapse_type
    decay / dephase select one dissipator."""
    text = synthetic_cfg([2, 2, 2]).replace("crosskerr = 0.001", "crosskerr = 0.01, 0.02").replace("decay_time = 80.0,80.0,80.0", "decay_time = 70.0, 0.0")
    sp = config.build_spec(config.parse_config_text(text))
    assert list(sp.system.crosskerr[:3]) == [0.01, 0.02, 0.02]
    assert list(sp.system.decay_time[:3]) == [70.0, 0.0, 0.0]
    assert list(sp.system.dephase_time[:3]) == [26.0, 26.0, 26.0]
    for collapse, want in (("decay", 1), ("dephase", 2), ("both", 3)):
        sp = synthetic_spec([2, 2], collapse=collapse)
        assert sp.system.lindblad_type == want == capi.LINDBLAD[collapse] and sp.lindblad
    assert synthetic_spec([2, 2], lindblad=False, collapse="decay").system.lindblad_type == capi.LINDBLAD["none"]


def _swapped(values, i, j):
    v = list(values)
    v[i], v[j] = v[j], v[i]
    return v


def _witnesses(nl, lindblad, collapse):
    """(name, keyword, the two entries exchanged) for every exchange that this system can see."""
    Q = len(nl)
    npairs = Q * (Q - 1) // 2
    out = []
    if npairs >= 2:
        out += [("a crosskerr", "crosskerr", 0, npairs - 1), ("b Jkl", "jkl_pairs", 0, npairs - 1)]
    if lindblad and collapse in ("dephase", "both"):
        out.append(("c dephase_time", "dephase_time", 0, Q - 1))
    if lindblad and collapse in ("decay", "both"):
        out.append(("d decay_time", "decay_time", 0, Q - 1))  # (both decay: the oscillator without decay is number 1 of three or more)
    deep = [k for k in range(Q) if nl[k] >= 3]  # a^+a^+aa vanishes on two levels
    if len(deep) >= 2:
        out.append(("e selfkerr", "selfkerr", deep[0], deep[-1]))
    return out


# 3x3x2 rather than 3x2x2: two oscillators with a third level, so that exchanged self-Kerr constants show with three oscillators too;
# 2x3x2x2 (six pairs, dim 576) has only one such oscillator, and exchange (e) does not apply to it
CASES = [pytest.param(nl, True, c, id="x".join(map(str, nl)) + "-" + c) for nl in ([3, 4], [3, 3, 2], [2, 3, 2, 2]) for c in ("decay", "dephase", "both")]
CASES.append(pytest.param([2, 2, 3, 2], False, "both", id="2x2x3x2-schroedinger"))


def test_every_exchange_is_witnessed_by_some_case():
    seen = {w[0] for c in CASES for w in _witnesses(*c.values)}
    assert seen == {"a crosskerr", "b Jkl", "c dephase_time", "d decay_time", "e selfkerr"}
    for c in CASES:
        nl, lindblad, collapse = c.values
        if lindblad and len(nl) >= 3:
            assert {w[0][0] for w in _witnesses(*c.values)} >= {"a", "b"} | ({"c"} if collapse != "decay" else set()) | ({"d"} if collapse != "dephase" else set())
    assert "e selfkerr" in {w[0] for w in _witnesses([3, 3, 2], True, "both")} and "e selfkerr" in {w[0] for w in _witnesses([3, 4], True, "both")}


@pytest.mark.parametrize("detuned", [True, False], ids=["eta0", "eta"])
@pytest.mark.parametrize("nl,lindblad,collapse", CASES)
def test_oracle_operator_with_unequal_constants_is_the_master_equation(nl, lindblad, collapse, detuned):
    kw = dict(lindblad=lindblad, collapse=collapse, detuned=detuned, ntime=5, **unequal_constants(len(nl)))
    sp = synthetic_spec(nl, **kw)
    orc = Oracle(sp)
    orc.set_params(40.0 * sp.params0)
    t, dim = 0.02, orc.dim
    pq = orc.eval_controls(np.array([t]))[0]
    assert np.abs(pq).min() > 1e-3, pq  # every p_k, q_k takes part
    x = np.random.default_rng(1).standard_normal(2 * dim)
    plain = None
    for tr in (False, True):
        got = orc.apply_rhs(t, x, transpose=tr)[0]
        want = master_equation_rhs(sp, pq, t, x, transpose=tr)
        err = np.abs(got[:dim] + 1j * got[dim:] - want).max() / np.abs(want).max()
        print(f"transpose={tr}: max |oracle - master equation| / max = {err:.2e}")
        np.testing.assert_allclose(got[:dim] + 1j * got[dim:], want, rtol=0, atol=1e-13 * np.abs(want).max())
        plain = want if plain is None else plain
    orc.close()
    # the fixture can see an exchanged index
    for name, key, i, j in _witnesses(nl, lindblad, collapse):
        assert kw[key][i] != kw[key][j]
        other = synthetic_spec(nl, **{**kw, key: _swapped(kw[key], i, j)})
        moved = np.abs(master_equation_rhs(other, pq, t, x) - plain).max() / np.abs(plain).max()
        print(f"{name} of {i} and {j} exchanged: moves the operator by {moved:.2e} of its maximum")
        assert moved >= WITNESS, name


def test_oracle_gradient_with_unequal_constants_matches_finite_differences():
    """3x2x2 Lindblad under collapse_type decay (oscillator 1 does not decay), every pair coupled, penalties on."""
    sp = synthetic_spec([3, 2, 2], lindblad=True, collapse="decay", detuned=True, ntime=10, nspline=6, penalties=True, maxiter=30, **unequal_constants(3))
    orc = Oracle(sp)
    _, g = orc.evalGradF(sp.params0)
    rng = np.random.default_rng(3)
    for i in rng.choice(sp.params0.size, 6, replace=False):
        e = np.zeros_like(sp.params0)
        e[i] = 1e-6
        fd = (orc.evalF(sp.params0 + e)[0]["objective"] - orc.evalF(sp.params0 - e)[0]["objective"]) / 2e-6
        assert fd == pytest.approx(g[i], rel=2e-5, abs=1e-9)
    orc.close()
