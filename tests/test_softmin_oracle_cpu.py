"""tests/softmin_oracle.py checked on its own, without a GPU: reduce against the plain definition in
np.longdouble and against the project's float64 softmin and shard combine; the fp32 restatement of the
kernels' combine inside the derived bound for every design and layout the GPU file uses; and each
planted mistake outside the bound on the designs named for it.  The worst err / bound per design is
printed (pytest -s) and, with SOFTMIN_ENVELOPE_LOG set, appended to that file."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import softmin_oracle as SO
from oracle import mppi_oracle as O

LAYOUTS, scene_and_pool = SO.LAYOUTS, SO.scene_and_pool


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("SOFTMIN_ENVELOPE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def check_design(d, pool, sc, lam, lay, model, tag, S=None, emu_lay=None):
    """The emulation inside the bound and the design's mistakes outside it; returns the ratios."""
    window = SO.SAVGOL[model]
    eps = d.noise(pool)
    S = d.costs(pool) if S is None else S
    red = SO.reduce(S, eps, lam, window, 2, sc.u0)
    bnd = SO.bounds(red, eps, lay)
    lay = lay if emu_lay is None else emu_lay   # (the layout the emulation runs; the bound keeps its own)
    emu = SO.emulate_fp32(S, eps, lam, lay, window, 2, sc.u0)
    assert emu["rho"] == np.float32(red.rho)
    r = SO.ratios(emu, red, bnd)
    _log(dict(side="cpu", case=tag, design=d.name, **{k: round(v, 4) for k, v in r.items()}))
    assert max(r.values()) <= 1.0, (tag, d.name, r)
    for m in d.exposes:
        bad = SO.ratios(SO.emulate_fp32(S, eps, lam, lay, window, 2, sc.u0, mistake=m), red, bnd)
        assert SO.exposed(bad, m) > 1.0, (tag, d.name, m, bad)
    return red, emu, r


# ------------------------------------------------------------------------------------------- reduce
def test_reduce_matches_the_definition_in_longdouble():
    rng = np.random.default_rng(3)
    for K, H, A, lam, spread in [(7, 8, 3, 0.1, 1.0), (300, 32, 7, 1e-3, 0.05), (64, 12, 4, 1e4, 1e5), (5, 8, 3, 1e30, 10.0)]:
        S = (40.0 + spread * rng.random(K)).astype(np.float32)
        S[rng.integers(K)] = np.inf if K > 5 else S[0]
        eps = rng.normal(0, 1, (K, H, A)).astype(np.float32)
        u = rng.normal(0, 1, (H, A)).astype(np.float32)
        taps = SO.savgol_taps(5, 2)
        r = SO.reduce(S, eps, lam, 5, 2, u)
        L = np.longdouble
        Sl, fin = S.astype(L), np.isfinite(S)
        e = np.where(fin, np.exp(-(np.where(fin, Sl, Sl[fin].min()) - Sl[fin].min()) / L(lam)), L(0))
        w = e / e.sum()
        raw = (w[:, None, None] * eps.astype(L)).sum(0)
        pad = np.concatenate([raw[:2][::-1], raw, raw[-2:][::-1]])
        sm = sum(L(taps[::-1][j]) * pad[j:j + H] for j in range(5))
        assert r.rho == float(S[fin].min())
        np.testing.assert_allclose(r.w, w.astype(np.float64), rtol=1e-12, atol=0)
        np.testing.assert_allclose(r.eta, float(e.sum()), rtol=1e-13)
        np.testing.assert_allclose(r.ess, float(e.sum() ** 2 / (e * e).sum()), rtol=1e-13)
        np.testing.assert_allclose(r.w_eps_raw, raw.astype(np.float64), rtol=0, atol=1e-13 * np.abs(eps).max())
        np.testing.assert_allclose(r.w_eps, sm.astype(np.float64), rtol=0, atol=1e-13 * np.abs(eps).max())
        np.testing.assert_allclose(r.u_prev_out, (u.astype(L) + sm).astype(np.float64), rtol=0, atol=1e-12)
        r2 = SO.reduce(S, eps, lam, 5, 2, u, dtype=np.longdouble)
        np.testing.assert_allclose(r2.w_eps.astype(np.float64), r.w_eps, rtol=0, atol=1e-13 * np.abs(eps).max())


def test_reduce_matches_the_float64_oracle():
    rng = np.random.default_rng(5)
    K, H, A, lam = 96, 32, 3, 0.1
    S = (30 + 2 * rng.random(K)).astype(np.float32)
    eps = rng.normal(0, 1, (K, H, A)).astype(np.float32)
    u = np.zeros((H, A), np.float32)
    r = SO.reduce(S, eps, lam, 5, 2, u)
    with O.float64_everywhere():
        S64, e64 = torch.tensor(S.astype(np.float64)), torch.tensor(eps.astype(np.float64))
        w = O.softmin(S64, lam)
        raw = torch.sum(w.view(-1, 1, 1) * e64, dim=0)
        parts = [O.shard_partial(S64[i:i + 32], e64[i:i + 32], lam) for i in (0, 32, 64)]
        comb = O.combine_partials(parts, lam)
    np.testing.assert_allclose(r.w, w.numpy(), rtol=1e-12)
    np.testing.assert_allclose(r.w_eps_raw, raw.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r.w_eps_raw, comb.numpy(), rtol=0, atol=1e-13)
    # the symmetric pad and the taps: the float64 savgol with the float64 solve of the same taps
    with O.float64_everywhere():
        sm = O.savgol(raw, 5, 2).numpy()
    np.testing.assert_allclose(r.w_eps, sm, rtol=0, atol=2e-7 * np.abs(sm).max())   # (fp32 taps against float64 ones)


def test_reduce_refuses_what_it_cannot_reduce():
    eps, u = np.zeros((2, 8, 3), np.float32), np.zeros((8, 3), np.float32)
    with pytest.raises(ValueError):
        SO.reduce(np.array([np.inf, np.inf], np.float32), eps, 0.1, 5, 2, u)
    with pytest.raises(ValueError):
        SO.reduce(np.array([1.0, np.nan], np.float32), eps, 0.1, 5, 2, u)


# ------------------------------------------------------------------------------ the designs themselves
def test_the_pool_holds_what_the_designs_assume():
    for model, H, lam in (("drone", 32, 0.1), ("drone", 32, 1e-3), ("drone", 32, 1e4), ("arm", 32, 0.1), ("wholebody", 64, 0.1)):
        _, pool = scene_and_pool(model, H, lam)
        want = np.array((0.0,) + SO.STAIR_X[1:] + SO.FAR_X + SO.NEAR_X)
        assert pool.best == 0 and pool.x[0] == 0.0
        np.testing.assert_allclose(pool.x, want, rtol=0, atol=0.02 + 1e-6 * pool.cost.max() / lam)
        assert (pool.x[pool.far] >= SO.FAR + 30).all()
        n = pool.noise(np.arange(len(pool.x)))
        assert len({n[i].tobytes() for i in range(len(n))}) >= len(n) - 1   # P distinct rows (x = 150 is wanted twice, and may come out of one profile)


def test_a_drone_row_scaled_by_1e20_costs_inf_not_nan():
    sc, pool = scene_and_pool("drone", 32, 0.1)
    rows = torch.tensor(np.stack([pool.noise([1])[0] * np.float32(1e20), pool.noise([1])[0]]))
    r = O.drone_step(sc.state[:3], sc.state[3:], torch.tensor(sc.u0), rows, SO.DRONE_TARGET)
    S = r["S"].numpy()
    assert S[0] == np.inf and np.isfinite(S[1])
    assert np.isfinite(rows.numpy()).all()


# ------------------------------------------------------------ the emulation inside the bound, mistakes outside
@pytest.mark.parametrize("tag,model,kw,lam", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_emulation_inside_the_bound_and_mistakes_outside(tag, model, kw, lam):
    lay = SO.layout_of(model=model, **kw)
    sc, pool = scene_and_pool(model, kw["n_horizon"], lam)
    K = kw["n_samples"]
    worst = 0.0
    for d in SO.designs(pool, K, lay, lam_is_default=(lam == 0.1), inf=(model == "drone" and kw["n_horizon"] == 32)):
        red, emu, r = check_design(d, pool, sc, lam, lay, model, tag)
        worst = max(worst, max(r.values()))
        if d.exact == "one_hot":
            k = int(np.argmax(red.w))
            assert emu["eta"] == 1.0 and emu["ess"] == 1.0 and emu["w"][k] == 1.0 and np.count_nonzero(emu["w"]) == 1
            assert np.array_equal(emu["w_eps_raw"], d.noise(pool)[k])
        if d.exact == "tied":
            assert emu["eta"] == K
        if d.inf is not None:
            assert all(np.isfinite(np.asarray(v)).all() for v in emu.values())
    assert worst > 0.0   # (the bound is not slack by orders of magnitude everywhere: see the log)


def test_offset_design_and_the_unshifted_exponential():
    """rho ~ 1e7 (the drone 56 m away), lambda = 10: the gaps are a few ulps of S (one ulp = 0.1 lambda)."""
    lam = 10.0
    sc = SO.drone_scene(lam, 32, far=float(np.sqrt(1e3)))
    pool = SO.make_pool(sc.cost_fn, sc.profiles, lam)
    assert 5e6 < pool.cost.min() < 5e7
    lay = SO.layout_of(model="drone", n_samples=272, n_horizon=32)
    for d in SO.designs(pool, 272, lay, lam_is_default=False):
        if d.name in ("staircase", "two_tied_far_apart"):
            d.exposes = d.exposes + ("unshifted",)
            check_design(d, pool, sc, lam, lay, "drone", "drone-offset")


def test_shards_exchanges_and_uniform_weights():
    """Two shards of 64 (the winner in shard 1, shard 0 entirely +inf, the staircase across both), the
    one-rank peer and native-communicator layouts on the staircase (their bound constants; the emulation is
    the plain engine's, which one rank reproduces: f = exp(0) = 1), and lambda = 1e30 (uniform)."""
    sc, pool = scene_and_pool("drone", 32, 0.1)
    one = SO.layout_of(model="drone", n_samples=64, n_horizon=32)
    lay = dataclasses.replace(one, shards=2)
    for d in SO.shard_designs(pool, one):
        red, emu, _ = check_design(d, pool, sc, 0.1, lay, "drone", "drone-shards2")
        if d.inf is not None:
            assert all(np.isfinite(np.asarray(v)).all() for v in emu.values())
        if d.exact == "one_hot":
            assert emu["eta"] == 1.0 and emu["ess"] == 1.0 and np.array_equal(emu["w_eps_raw"], d.noise(pool)[64 + 37])
    lay1 = SO.layout_of(model="drone", n_samples=272, n_horizon=32)
    stairs = SO.place_staircase(pool, 272, lay1)
    for kind, bl in (("peer", dataclasses.replace(lay1, peer=1)), ("comm", dataclasses.replace(lay1, shards=2))):
        d = SO.Design("staircase", stairs, ("per_record", "eta2_f", "edge_pad"))
        check_design(d, pool, sc, 0.1, bl, "drone", f"drone-K272-{kind}", emu_lay=lay1)
    d = SO.Design("staircase", stairs, ("lam01", "edge_pad"))
    red, emu, _ = check_design(d, pool, sc, 1e30, lay1, "drone", "drone-K272-lam1e30")
    assert np.abs(emu["w"].astype(np.float64) - 1.0 / 272).max() <= SO.bounds(red, d.noise(pool), lay1).w.max()
