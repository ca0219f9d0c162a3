"""tests/aerial_oracle.py held to itself, without a GPU: the fp32 restatement of the composition passes the
derived bounds on every design and shape of tests/test_gpu_aerial.py, each planted mistake fails at least one
of them (the assert_case_can_fail pattern: a check that could not fail shows nothing), and the oracle's own
numbers stay inside the exclusion caps on those inputs."""
import numpy as np
import pytest

import aerial_oracle as A


@pytest.fixture(scope="module")
def runs(kinova_chain):
    """Per (case, vehicle): (design, u, eps, oracle)."""
    out = {}
    for case in A.CASES:
        for v, (d, u, eps) in enumerate(case.vehicles()):
            out[(case.tag, v)] = (case, d, u, eps, A.rollout(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal))
    return out


def test_reach_is_about_a_metre(kinova_chain):
    assert 0.8 < A.chain_reach(kinova_chain) < 1.5


def test_caps_hold_on_every_design(runs):
    for key, (case, d, u, eps, ao) in runs.items():
        ro = ao.base
        excluded = 1.0 - ao.valid[:, -1].mean()
        m3 = np.broadcast_to(ro.valid[..., None], ro.circ.shape)
        circular = (ro.circ & m3).sum() / max(1, m3.sum())
        print(key, "excluded", excluded, "circular", circular, "max |m20|", float(np.abs(ao.m20).max()),
              "max b_ee", float(np.where(ao.valid[..., None], ao.b_ee, 0).max()), "max b_S / S", float(np.max(ao.b_S[ao.valid[:, -1]] / ao.S[ao.valid[:, -1]])))
        assert excluded <= A.EXCLUDED_CAP, (key, excluded)
        assert circular <= A.CIRCULAR_CAP, (key, circular)
        assert np.isfinite(ao.S).all() and np.isfinite(ao.b_S[ao.valid[:, -1]]).all()


def test_state_is_tilted_and_turning():
    for d in A.DESIGNS:
        assert 0.4 <= abs(d.x[3]) <= 0.6 and 0.4 <= abs(d.x[4]) <= 0.6, d.name
        assert max(abs(w) for w in d.v[3:]) >= 1.8, d.name


def test_restatement_passes_the_bounds(kinova_chain, runs):
    for key, (case, d, u, eps, ao) in runs.items():
        em = A.emulate(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal)
        r = A.compare(ao, em["base"], em["q"], em["ee"], em["S"])
        print(key, r)
        assert r.worst() <= 1.0, (key, r)


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_each_planted_mistake_fails_a_design(kinova_chain, runs, variant):
    worst = {}
    for key, (case, d, u, eps, ao) in runs.items():
        em = A.emulate(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal, variant=variant)
        r = A.compare(ao, em["base"], em["q"], em["ee"], em["S"])
        worst[key] = max(r.q, r.ee, r.rot, r.S)
    print(variant, worst)
    assert max(worst.values()) > 1.0, (variant, worst)
    if variant == "fixed_attitude":   # the mistake the model exists to remove: visible in every case
        assert min(worst.values()) > 1.0, worst


def test_plan_row_is_the_zero_noise_sample(kinova_chain):
    """cost_t sums to S and pos_err is the L1 distance: what the plan test compares."""
    d = A.DESIGNS[0]
    u, _ = d.inputs(1, 20)
    ao = A.rollout(kinova_chain, u, np.zeros((1, 20, A.NA), np.float32), d.state, d.tpos, d.tquat, d.cfg)
    assert abs(ao.cost_t[0].sum() - ao.S[0]) <= 1e-9 * ao.S[0]
    want = np.abs(ao.ee[0, :, :3, 3] - np.asarray(d.tpos, np.float32).astype(np.float64)).sum(-1)
    assert np.allclose(ao.pos_err[0], want, rtol=0, atol=1e-12)
