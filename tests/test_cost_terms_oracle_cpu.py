"""tests/cost_terms_oracle.py on its own, with no GPU: on every case of tests/test_gpu_cost_terms.py the fp32
restatement of the kernels stays inside the oracle's bounds, each planted mistake a case is declared to expose
leaves them by at least 10 x, every planted mistake is exposed by some case, the limit cases keep enough samples on
each side of the flag, and every enabled term stands at least 100 x above its own bound on half of the samples."""
import functools

import numpy as np
import pytest

import cost_terms_oracle as CT

CASES = CT.ROLLOUT + CT.PLAN
EXPOSE = 10.0
SIZE = 100.0


def _vehicles(case):
    return range(case.V)


@functools.lru_cache(maxsize=None)
def _setup(tag, v):
    case = CT.BY_TAG[tag]
    inp = case.inputs(v)
    plan = case in CT.PLAN
    return case, inp, CT.oracle(inp, zero_noise=plan), plan


@pytest.mark.parametrize("case", CASES, ids=[c.tag for c in CASES])
def test_restatement_inside_and_mistakes_outside(case):
    for v in _vehicles(case):
        _, inp, o, plan = _setup(case.tag, v)
        r = CT.compare(o, CT.emulate(inp, zero_noise=plan))
        assert max(r.values()) <= 1.0, (case.tag, v, r)
        for m in CT.declared(case, inp.lay, v):
            bad = CT.compare(o, CT.emulate(inp, m, zero_noise=plan))
            assert CT.exposed(bad, m) >= EXPOSE, (case.tag, v, m, bad)


def test_every_mistake_is_exposed_by_some_case():
    seen = set()
    for case in CASES:
        lay = CT.layout_of(**case.config())
        for v in _vehicles(case):
            seen.update(CT.declared(case, lay, v))
    assert seen == set(CT.MISTAKES), set(CT.MISTAKES) - seen


@pytest.mark.parametrize("case", [c for c in CT.ROLLOUT if "limit" in c.terms], ids=lambda c: c.tag)
def test_limit_cases_keep_both_sides_of_the_flag(case):
    for v in _vehicles(case):
        _, inp, o, _ = _setup(case.tag, v)
        K = case.K
        hit, clear = int((o.kept & o.hit).sum()), int((o.kept & ~o.hit).sum())
        print(f"{case.tag} v{v}: excluded {o.excluded} of {K}; hit {hit}, clear {clear}")
        assert o.excluded <= CT.EXCLUDED_CAP * K
        assert hit >= 0.1 * K and clear >= 0.1 * K, (case.tag, hit, clear)
        if len(case.terms) == 1:   # (alone, the term is zero on the clear side: the hit side is its half)
            assert hit >= 0.5 * K, (case.tag, hit)


@pytest.mark.parametrize("case", CASES, ids=[c.tag for c in CASES])
def test_every_enabled_term_stands_above_its_bound(case):
    for v in _vehicles(case):
        _, inp, o, plan = _setup(case.tag, v)
        assert set(o.val) == set(case.terms)
        for name in case.terms:   # (a vehicle without a table tracks zeros: ||q||^2, as large as any)
            big = np.abs(o.val[name]) >= SIZE * o.bnd[name]
            assert big.sum() >= 0.5 * len(big), (case.tag, v, name, float(np.median(np.abs(o.val[name]) / o.bnd[name])))


@pytest.mark.parametrize("case", CT.PLAN, ids=[c.tag for c in CT.PLAN])
def test_plan_cases_cross_the_limits_between_steps(case):
    """The plan's path keeps every step clear of the limit rule, crosses the upper limit first (steps with one joint
    out), then the lower (steps with two), and its warm start and table are not zero."""
    _, inp, o, _ = _setup(case.tag, 0)
    out = ((o.q < inp.qlo) | (o.q > inp.qhi))[0].sum(-1)
    assert o.kept_t.all() and o.hit[0] and inp.tables.any() and inp.u.any()
    assert (out == 0).sum() >= case.H // 4 and (out == 1).sum() >= case.H // 8 and (out == 2).sum() >= case.H // 8, out


def test_bound_counts_follow_the_layout():
    """The sum's share of the bound grows with the scan depth and the chunks, and with nothing else."""
    case = CT.BY_TAG["arm-k32h96-action"]
    inp = case.inputs()
    assert (inp.lay.L, inp.lay.nch, inp.lay.levels) == (64, 2, 7)
    o = CT.oracle(inp)
    x = o.val_t["action"]
    want = CT.SECOND * (x * CT.U * (2 + 7 + 4)).sum(-1) + CT.SECOND * 7 * CT.U * x.sum(-1)
    assert np.allclose(o.bnd["action"], want, rtol=1e-12)
    looped = CT.BY_TAG["arm-looped-covar"].inputs()
    assert (looped.lay.L, looped.lay.R, looped.lay.nw, looped.lay.nb, looped.lay.iters) == (32, 2, 2, 8, 2)


def test_inverse_and_discount_are_formed_here():
    """Sigma^-1 and gamma^t of the oracle against the definition, not against the library's tables."""
    case = CT.BY_TAG["wb-k32h64-covar"]
    s = case.sigma32().astype(np.float64)
    assert np.any(s[~np.eye(10, dtype=bool)] != 0) and np.all(np.linalg.eigvalsh(s) > 0)
    assert np.allclose(np.linalg.inv(s) @ s, np.eye(10), atol=1e-12)
    inp = case.inputs()
    o = CT.oracle(inp)
    v = inp.u.astype(np.float64)[None] + inp.eps.astype(np.float64)
    want = case.par.w_cov * np.einsum("ha,ab,khb->k", inp.u.astype(np.float64), np.linalg.inv(s), v)
    assert np.allclose(o.val["covar"], want, rtol=1e-12)
    assert case.par.w_cov == float(np.float32(float(np.float32(0.3)) * (0.1 * (1.0 - float(np.float32(0.25))))))
