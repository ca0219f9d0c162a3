"""The control step's reduction on the GPU against tests/softmin_oracle.py: one control call with
injected noise per design, then get_costs, get_weights, get_weighted_noise (the READBACK launch),
get_u_prev and the stats compared with reduce(S_gpu, eps, lambda) under the derived bound (the module's
docstring: a, b, d counted from the kernels' operation chain; nothing here is tuned to what the kernels
give).  Each case runs the engine as shipped and with MPPI_GENERIC_KERNELS=1, asserts through
kernel_info() which finalize ran, and first asserts from the oracle alone that the mistakes named for
the design would fail it.  The designs place the minimum where the combine can lose it: the last lane
group, wave slot, record, the record past a chunk boundary, the other shard; records that lose by more
than the exponent's range; +inf costs without a NaN.

Injected noise always runs through HIP launches (mppi_step takes native dispatch only for device noise),
so the placed designs cannot reach the native path; MPPI_DISPATCH=hip|aql is swept by the device-noise
cases (natural costs over the lambda sweep; the exact one-hot case with lambda set from the natural costs'
top-two gap) and the quiet roles.
The quadrotor's rollout (mppi_rollout_quad.hip) has its own one-pass block combine, counted on its own
(Layout.quad).
With SOFTMIN_ENVELOPE_LOG set every err / bound is appended to that file (profiles/r19/softmin_envelope)."""
import dataclasses
import json
import os

import numpy as np
import pytest

import softmin_oracle as SO

pytestmark = pytest.mark.gpu

GENERIC = "_Z10k_finalizeILi"
ROLE = "_Z12k_finalize_sILi"
GID = {"arm": 1, "drone": 2, "quadrotor": 3, "wholebody": 4}
TABLE_H = {"arm": 32, "drone": 32, "quadrotor": 32, "wholebody": 64}
FAMILIES = (("shipped", {}), ("generic", {"MPPI_GENERIC_KERNELS": "1"}))
LAMBDAS = (1e-3, 0.1, 10.0, 1e4, 1e30)


def _engine(monkeypatch, env, **cfg):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read at mppi_create
    try:
        e = Engine(make_config(device=0, seed=31, **cfg))
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return e


def _prepare(e, sc):
    for v in range(e.V):
        e.set_target(sc.target[0], sc.target[1], vehicle=v)
    e.set_state(np.tile(sc.state, (e.V, 1)))


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("SOFTMIN_ENVELOPE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _finalize_ran(e, model, H, nrec, family, window=None):
    info = e.kernel_info()
    call = info.split("call:")[-1]
    if family == "shipped" and H == TABLE_H[model] and window in (None, SO.SAVGOL[model]):
        nt = 128 if nrec <= 128 else 256 if nrec <= 256 else 512
        assert f"finalize {ROLE}{nt}ELi" in call and f"ELi{GID[model]}E" in call, info
    else:
        assert ROLE not in call and f"finalize {GENERIC}" in call, info


def _outputs(e, ret, tag, name):
    """What the control call itself returned (the FINAL kernel's tail, not the READBACK launch): finite,
    and u0 the first row of the new warm start bit for bit."""
    out, u0, _ = ret
    assert np.isfinite(out).all() and np.isfinite(u0).all(), (tag, name, "non-finite step output", out, u0)
    np.testing.assert_array_equal(u0, e.get_u_prev()[:, 0, :], err_msg=f"{tag} {name}: u0 is not u_prev[0]")


def _compare(S, eps, got, st, lam, lay, model, u0, tag, name, family, exposes=(), exact=None, inf=None, place=None):
    """One vehicle's readbacks against the oracle; returns (reduced, ratios)."""
    window = SO.SAVGOL[model]
    if place is not None:   # copies of one pool row cost the same bits
        for p in np.unique(place):
            sel = (place == p) if inf is None else (place == p) & ~inf
            assert len(np.unique(S[sel])) <= 1, (tag, name, "copies of pool row", int(p), np.unique(S[sel]))
    if inf is not None:
        assert (S[inf] == np.inf).all() and np.isfinite(S[~inf]).all(), (tag, name, S)
    red = SO.reduce(S, eps, lam, window, 2, u0)
    bnd = SO.bounds(red, eps, lay)
    if family == "shipped":   # from the oracle alone: the design would catch its mistakes
        for m in exposes:
            bad = SO.ratios(SO.emulate_fp32(S, eps, lam, dataclasses.replace(lay, peer=0), window, 2, u0, mistake=m), red, bnd)
            assert SO.exposed(bad, m) > 1.0, (tag, name, "does not expose", m, bad)
    assert np.float32(st.rho) == np.float32(red.rho), (tag, name, st.rho, red.rho)
    assert not st.nonfinite, (tag, name, "stats.nonfinite")
    got = dict(got, eta=st.eta, ess=st.ess)
    assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in got.values()), (tag, name, "non-finite output")
    r = SO.ratios(got, red, bnd)
    _log(dict(side="gpu", case=tag, family=family, design=name, **{k: round(v, 4) for k, v in r.items()}))
    assert max(r.values()) <= 1.0, (tag, name, family, r)
    K = len(S)
    if exact == "one_hot":
        assert np.sort(red.x)[1] >= SO.FAR, (tag, name, "the design's gap did not survive the fp32 costs", np.sort(red.x)[:3])
        k = int(np.argmin(S))
        assert st.eta == 1.0 and st.ess == 1.0, (tag, name, st)
        assert got["w"][k] == 1.0 and np.count_nonzero(got["w"]) == 1, (tag, name)
        assert np.array_equal(got["w_eps_raw"], eps[k]), (tag, name, "w_eps_raw is not the winner's eps")
    if exact == "tied":
        assert st.eta == float(K), (tag, name, st.eta)
    return red, r


def _run_designs(e, sc, pool, per_vehicle, lam, lay, model, tag, family):
    """One control call; per_vehicle[v] is vehicle v's design."""
    eps = np.stack([d.noise(pool) for d in per_vehicle])
    e.set_u_prev(np.tile(sc.u0, (e.V, 1, 1)))
    ret = e.step(np.tile(sc.state, (e.V, 1)), eps)
    stats = ret[2]
    _outputs(e, ret, tag, "/".join(d.name for d in per_vehicle))
    S, w, (raw, sm), u = e.get_costs(), e.get_weights(), e.get_weighted_noise(), e.get_u_prev()
    for v, d in enumerate(per_vehicle):
        got = dict(w=w[v], w_eps_raw=raw[v], w_eps=sm[v], u_prev=u[v])
        _compare(S[v], eps[v], got, stats[v], lam, lay, model, sc.u0, tag, d.name + (f"/v{v}" if e.V > 1 else ""), family,
                 d.exposes, d.exact, d.inf, d.place)


# --------------------------------------------------------------- records, groups, lane maps, lambda: the pool designs
@pytest.mark.parametrize("tag,model,kw,lam", SO.LAYOUTS, ids=[c[0] for c in SO.LAYOUTS])
def test_pool_designs_inside_the_bound(monkeypatch, tag, model, kw, lam):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lay = SO.layout_of(model=model, lam=lam, **kw)
    sc, pool = SO.scene_and_pool(model, kw["n_horizon"], lam)
    K = kw["n_samples"]
    ds = SO.designs(pool, K, lay, lam_is_default=(lam == 0.1), inf=(model == "drone" and kw["n_horizon"] == 32))
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, model=model, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        for d in ds:
            _run_designs(e, sc, pool, [d], lam, lay, model, tag, family)
        _finalize_ran(e, model, kw["n_horizon"], lay.nb, family)
        e.close()


def test_uniform_weights_at_lambda_1e30(monkeypatch):
    """lambda = 1e30 on the lambda = 0.1 staircase: every weight 1/K to the bound."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lam, K = 1e30, 272
    kw = dict(model="drone", n_samples=K, n_horizon=32)
    lay = SO.layout_of(lam=lam, **kw)
    sc, pool = SO.scene_and_pool("drone", 32, 0.1)
    d = SO.Design("staircase", SO.place_staircase(pool, K, lay), ("lam01", "edge_pad"))
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        _run_designs(e, sc, pool, [d], lam, lay, "drone", "drone-K272-lam1e30", family)
        red = SO.reduce(e.get_costs()[0], d.noise(pool), lam, 5, 2, sc.u0)
        assert np.abs(e.get_weights()[0].astype(np.float64) - 1.0 / K).max() <= SO.bounds(red, d.noise(pool), lay).w.max()
        e.close()


def test_offset_costs(monkeypatch):
    """rho ~ 1e7, lambda = 10: cost gaps of a few ulps of S; the unshifted exponential would give 0 / 0."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lam, K = 10.0, 272
    kw = dict(model="drone", n_samples=K, n_horizon=32)
    lay = SO.layout_of(lam=lam, **kw)
    sc = SO.drone_scene(lam, 32, far=float(np.sqrt(1e3)))
    pool = SO.make_pool(sc.cost_fn, sc.profiles, lam)
    ds = [dataclasses.replace(d, exposes=d.exposes + ("unshifted",)) for d in SO.designs(pool, K, lay, False)
          if d.name in ("staircase", "two_tied_far_apart")]
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        for d in ds:
            _run_designs(e, sc, pool, [d], lam, lay, "drone", "drone-offset", family)
            assert 5e6 < e.get_costs()[0].min() < 5e7
        e.close()


def test_fleet_every_vehicle_its_own_placement(monkeypatch):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lam, K = 0.1, 48
    kw = dict(model="drone", n_samples=K, n_horizon=32, n_vehicles=3)
    lay = SO.layout_of(lam=lam, **kw)
    sc, pool = SO.scene_and_pool("drone", 32, lam)
    ds = SO.designs(pool, K, lay, inf=True)
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        for i in range(len(ds)):
            _run_designs(e, sc, pool, [ds[(i + v) % len(ds)] for v in range(3)], lam, lay, "drone", "drone-fleet3", family)
        _finalize_ran(e, "drone", 32, lay.nb, family)
        e.close()


def test_quadrotor_lane_map(monkeypatch):
    """Quadrotor H = 32, K = 48 (its own rollout kernel and block combine): random rows with natural costs
    at lambda = 0.1 and the exact designs made from the costs read back -- the best row against copies of
    rows at least 110 lambda above it."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lam, K, H = 0.1, 48, 32
    kw = dict(model="quadrotor", n_samples=K, n_horizon=H)
    lay = SO.Layout(R=16, nw=1, iters=1, nb=3, quad=True)   # one dynamics wave of 16 rollouts per record
    state = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0] + [0.0] * 6)
    rng = np.random.default_rng(11)
    rows = (rng.normal(0.0, 1.0, (K, H, 4)) * np.array([40.0, 0.3, 0.3, 0.3])).astype(np.float32)
    u0 = np.zeros((H, 4), np.float32)
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        e.set_target(SO.DRONE_TARGET)

        def call(eps, name, exact=None):
            e.set_u_prev(u0[None])
            ret = e.step(state, eps[None])
            st = ret[2]
            _outputs(e, ret, "quadrotor-K48", name)
            raw, sm = e.get_weighted_noise()
            got = dict(w=e.get_weights()[0], w_eps_raw=raw[0], w_eps=sm[0], u_prev=e.get_u_prev()[0])
            return _compare(e.get_costs()[0], eps, got, st[0], lam, lay, "quadrotor", u0, "quadrotor-K48", name, family,
                            exact=exact)
        red, _ = call(rows, "natural")
        order = np.argsort(red.x)
        far = order[red.x[order] >= red.x[order[0]] + 1.5 * SO.FAR]
        assert len(far) >= 2, red.x[order]
        for pos in (0, 15, 16, 47):
            place = far[np.arange(K) % len(far)]
            place[pos] = order[0]
            call(rows[place], f"winner_at_{pos}", "one_hot")
        call(rows[np.full(K, order[0])], "all_tied", "tied")
        _finalize_ran(e, "quadrotor", H, 3, family)
        e.close()


# ------------------------------------------------------------------ device noise: natural costs, both dispatch paths
@pytest.mark.parametrize("dispatch", ["hip", "aql"])
@pytest.mark.parametrize("model,K,H", [("arm", 4096, 32), ("wholebody", 2048, 64)])
def test_natural_costs_over_lambda(monkeypatch, model, K, H, dispatch):
    sc = SO.chain_scene(model, H)
    kw = dict(model=model, n_samples=K, n_horizon=H, store_noise=True)
    if model == "arm":
        kw["state_f64"] = True
    for lam in LAMBDAS:
        for family, env in FAMILIES:
            _natural_call(monkeypatch, sc, kw, lam, dispatch, family, env)


def _natural_call(monkeypatch, sc, kw, lam, dispatch, family, env, exact=None):
    """One control call with device noise on one dispatch path against the oracle over the stored noise;
    returns the costs."""
    model, K, H = kw["model"], kw["n_samples"], kw["n_horizon"]
    lay = SO.layout_of(lam=lam, **kw)
    e = _engine(monkeypatch, dict(env, MPPI_DISPATCH=dispatch), lam=lam, **kw)
    _prepare(e, sc)
    e.set_u_prev(sc.u0[None])
    ret = e.step(sc.state)
    st = ret[2]
    _outputs(e, ret, f"{model}-K{K}-natural-{dispatch}-lam{lam:.3g}", family)
    assert e.dispatch_info().split("calls:")[-1].strip().startswith(dispatch), e.dispatch_info()
    S, eps = e.get_costs()[0], e.get_noise()[0]
    raw, sm = e.get_weighted_noise()
    got = dict(w=e.get_weights()[0], w_eps_raw=raw[0], w_eps=sm[0], u_prev=e.get_u_prev()[0])
    x = np.sort((S.astype(np.float64) - S.min()) / lam)
    _compare(S, eps, got, st[0], lam, lay, model, sc.u0, f"{model}-K{K}-natural-{dispatch}-lam{lam:.3g}",
             "natural" if exact is None else "natural_winner", family,
             exact=exact or ("one_hot" if x[1] >= SO.FAR else None))
    _finalize_ran(e, model, H, lay.nb, family)
    e.close()
    return S


@pytest.mark.parametrize("dispatch", ["hip", "aql"])
@pytest.mark.parametrize("model,K,H", [("arm", 4096, 32), ("wholebody", 2048, 64)])
def test_exact_winner_on_both_dispatch_paths(monkeypatch, model, K, H, dispatch):
    """The exact case where native dispatch can reach it: device noise, lambda set from the natural costs'
    own top-two gap (gap / 150, so every other sample is at least 110 lambda behind whatever the last ulp of
    S does): w one-hot, eta = ess = 1, w_eps_raw the winner's stored eps bit for bit, on both families."""
    sc = SO.chain_scene(model, H)
    kw = dict(model=model, n_samples=K, n_horizon=H, store_noise=True)
    if model == "arm":
        kw["state_f64"] = True
    S0 = _natural_call(monkeypatch, sc, kw, 0.1, dispatch, "generic", FAMILIES[1][1])
    top = np.sort(S0.astype(np.float64))
    assert top[1] > top[0], "the two best natural costs tie"
    lam = float(top[1] - top[0]) / 150.0
    for family, env in FAMILIES:
        S = _natural_call(monkeypatch, sc, kw, lam, dispatch, family, env, exact="one_hot")
        np.testing.assert_array_equal(S, S0)   # (the costs do not depend on lambda)


@pytest.mark.parametrize("dispatch", ["hip", "aql"])
@pytest.mark.parametrize("lam", LAMBDAS)
def test_quiet_roles_over_lambda(monkeypatch, lam, dispatch):
    """run_steps(3) (two quiet rollouts and quiet FINALs, then the full step) against three control calls
    on a twin with the same seed: u_prev bit for bit."""
    for model, K, H in (("arm", 272, 32), ("drone", 4096, 32)):
        sc = SO.chain_scene(model, H) if model == "arm" else SO.drone_scene(0.1, H)
        kw = dict(model=model, n_samples=K, n_horizon=H, lam=lam)
        a = _engine(monkeypatch, {"MPPI_DISPATCH": dispatch}, **kw)
        b = _engine(monkeypatch, {"MPPI_DISPATCH": dispatch}, **kw)
        for e in (a, b):
            _prepare(e, sc)
            e.set_u_prev(sc.u0[None])
        a.run_steps(3)
        a.synchronize()
        for _ in range(3):
            b.step(sc.state)
        assert np.isfinite(a.get_u_prev()).all()
        np.testing.assert_array_equal(a.get_u_prev(), b.get_u_prev(), err_msg=f"{model} lambda {lam:g} {dispatch}")
        info = a.kernel_info()
        assert "quiet finalize " + ROLE in info and "quiet rollout none" not in info, info
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("name", ["winner_in_shard_1", "shard_0_inf", "staircase"])
def test_two_shards_host_summed_slots(monkeypatch, name):
    """Two shard engines over 2 x 64 samples, their exchange slots summed on the host
    (test_shards_combine_like_one_engine), against the oracle over all 128."""
    import torch
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    lam, K, H = 0.1, 64, 32
    sc, pool = SO.scene_and_pool("drone", H, lam)
    one = SO.layout_of(model="drone", n_samples=K, n_horizon=H)
    lay = dataclasses.replace(one, shards=2)
    d = next(x for x in SO.shard_designs(pool, one) if x.name == name)
    place, inf, exposes, exact = d.place, d.inf, d.exposes, d.exact
    eps = d.noise(pool)
    for family, env in FAMILIES:
        shards = [_engine(monkeypatch, env, model="drone", n_samples=K, n_horizon=H, lam=lam, noise="injected",
                          shard_rank=r, shard_count=2) for r in range(2)]
        slot = shards[0].exchange_slot_floats()
        bufs = [torch.zeros(2 * slot, device="cuda") for _ in range(2)]
        dn = [torch.tensor(eps[r * K:(r + 1) * K][None]).cuda().contiguous() for r in range(2)]
        for sh, b, n in zip(shards, bufs, dn):
            _prepare(sh, sc)
            sh.set_u_prev(sc.u0[None])
            sh.bind_exchange(b.data_ptr())
            sh.rollout(n.data_ptr())
            sh.synchronize()
        total = bufs[0] + bufs[1]
        for sh, b in zip(shards, bufs):
            b.copy_(total)
            torch.cuda.synchronize()
            sh.finalize()
        outs = [sh.read_outputs() for sh in shards]
        for sh, o in zip(shards, outs):
            _outputs(sh, o, "drone-shards2", name)
        S = np.concatenate([sh.get_costs()[0] for sh in shards])
        w = np.concatenate([sh.get_weights()[0] for sh in shards])
        np.testing.assert_array_equal(shards[0].get_u_prev(), shards[1].get_u_prev())
        for r, sh in enumerate(shards):
            raw, sm = sh.get_weighted_noise()
            got = dict(w=w, w_eps_raw=raw[0], w_eps=sm[0], u_prev=sh.get_u_prev()[0])
            _compare(S, eps, got, outs[r][2][0], lam, lay, "drone", sc.u0, "drone-shards2", f"{name}/rank{r}",
                     family if r == 0 else "rank1-" + family, exposes, exact, inf, place)
        for sh in shards:
            sh.close()


@pytest.mark.parametrize("kind", ["peer", "comm"])
def test_one_rank_exchanges_on_the_staircase(monkeypatch, kind):
    """The one-rank peer engine (FINAL with the exchange) and the one-rank native communicator (pack,
    all-reduce, combine from slots) on the staircase."""
    from quadrotor_manipulator_mppi_amd.engine import Engine
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    if kind == "comm" and Engine.comm_available() is not None:
        pytest.skip("no native communicator: " + str(Engine.comm_available()))
    lam, K, H = 0.1, 272, 32
    kw = dict(model="drone", n_samples=K, n_horizon=H)
    one = SO.layout_of(lam=lam, **kw)
    lay = dataclasses.replace(one, peer=1) if kind == "peer" else dataclasses.replace(one, shards=2)
    sc, pool = SO.scene_and_pool("drone", H, lam)
    d = SO.Design("staircase", SO.place_staircase(pool, K, one), ("per_record", "eta2_f", "edge_pad") if kind == "peer" else ())
    eps = d.noise(pool)
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        if kind == "peer":
            e.peer_connect([e.peer_open()])
            for ph in (0, 1, 2):
                e.peer_probe(ph)
        else:
            e.comm_init(e.comm_unique_id())
        e.set_u_prev(sc.u0[None])
        ret = e.step(sc.state, eps[None])
        st = ret[2]
        _outputs(e, ret, f"drone-K272-{kind}", "staircase")
        raw, sm = e.get_weighted_noise()
        got = dict(w=e.get_weights()[0], w_eps_raw=raw[0], w_eps=sm[0], u_prev=e.get_u_prev()[0])
        _compare(e.get_costs()[0], eps, got, st[0], lam, lay, "drone", sc.u0, f"drone-K272-{kind}", "staircase", family,
                 d.exposes, None, None, d.place)
        if kind == "peer" and family == "shipped":
            assert f"finalize {ROLE}128ELi4ELi2E" in e.kernel_info(), e.kernel_info()   # kRolePeer
        e.close()


# ------------------------------------------------------------------------------------------- elites
@pytest.mark.parametrize("lam", LAMBDAS)
def test_elites_on_the_staircase(monkeypatch, lam):
    """get_elites(8): indices and costs exact (ascending in (cost, index)), weights within the per-sample
    bound, on both kernel families.  At lambda = 1e30 the lambda = 0.1 pool's staircase is placed (as in
    test_uniform_weights_at_lambda_1e30): every weight ties at 1/K and the choice rests on (cost, index) alone."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    K, H = 272, 32
    kw = dict(model="drone", n_samples=K, n_horizon=H)
    lay = SO.layout_of(lam=lam, **kw)
    sc, pool = SO.scene_and_pool("drone", H, 0.1 if lam == 1e30 else lam)
    d = SO.Design("staircase", SO.place_staircase(pool, K, lay))
    eps = d.noise(pool)
    for family, env in FAMILIES:
        e = _engine(monkeypatch, env, lam=lam, noise="injected", **kw)
        _prepare(e, sc)
        e.set_u_prev(sc.u0[None])
        _outputs(e, e.step(sc.state, eps[None]), f"drone-K272-elites-lam{lam:g}", "staircase")
        S = e.get_costs()[0]
        el = e.get_elites(n=8, traj=False)
        want = np.lexsort((np.arange(K), S))[:8]
        assert len(np.unique(S[want])) < 8, "the staircase's copies tie: the index decides among them"
        np.testing.assert_array_equal(el.idx[0], want)
        np.testing.assert_array_equal(el.S[0], S[want])
        red = SO.reduce(S, eps, lam, 5, 2, sc.u0)
        bw = SO.bounds(red, eps, lay).w
        assert np.isfinite(el.w[0]).all()
        err = np.abs(el.w[0].astype(np.float64) - red.w[want])
        _log(dict(side="gpu", case=f"drone-K272-elites-lam{lam:g}", family=family, design="staircase",
                  w=round(float(np.max(err / bw[want])), 4)))
        assert (err <= bw[want]).all(), (family, err, bw[want])
        _finalize_ran(e, "drone", H, lay.nb, family)
        e.close()
