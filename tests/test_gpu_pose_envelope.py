"""The forward kinematics and the pose cost of every rollout kernel form and of the plan kernel over
the joint, base and target envelope (tests/pose_envelope.py: the ray sweep, the three stages and
their references; tests/test_pose_envelope_cpu.py: the same cases on the oracle alone).

Every launch is K = 256 rollouts walking straight lines in joint space from the home posture to the
256 joint vectors of F3 ([-6, 6]^7, times 8 for the wound-up runs: |q| up to 48 rad), on F3's four
bases (two with roll and pitch).  Stage A (FK) and stage C (S under the default and under another set
of weights) run for every form; stage B (the orientation and the position norm alone, under weights
(0, 0, 0, 1) and (0, 0, 1, 0)) for the forms of B_FORMS against 16 targets -- the reference's, 8 of
F4's, the zero-error target and error rotations toward the gimbal singularity and yaw, roll = +-pi --
on the ray set and on a cluster of postures around rollout 5's.  The generic chain (ten joints: skew
axes, a prismatic joint, fixed joints in mid-chain, q_index out of order) must report chain_fast == 0.

The achieved maxima go to $MPPI_ACCURACY_OUT (``_envelope_<name>`` suffix) when it is set.
"""
import json
import os

import numpy as np
import pytest

import pose_envelope as P
import tracking_oracle as TO

pytestmark = pytest.mark.gpu

BASES = P.f3()[1]

FORMS = {
    # name: model, H, fp64 state, chain, full = every base and the wound-up run, expected chain_fast
    "arm64-h32": dict(model="arm", H=32, f64=True, full=True),          # C3: sin / cos ahead of the chain
    "arm32-h32": dict(model="arm", H=32, f64=False, full=True),         # arm32 unit, fp32 reduction
    "arm64-h64": dict(model="arm", H=64, f64=True, full=True),          # kin_joint, L = 64
    "arm32-h64": dict(model="arm", H=64, f64=False, full=True),
    "arm64-h100": dict(model="arm", H=100, f64=True),                   # two horizon chunks
    "revz64-h32": dict(model="arm", H=32, f64=True, env=True, fast=1),  # XC, the revolute-z loop
    "generic64-h32": dict(model="arm", H=32, f64=True, generic=True, fast=0),
    "generic32-h32": dict(model="arm", H=32, f64=False, generic=True, fast=0),
    "wb-h64": dict(model="wholebody", H=64, f64=False, full=True),      # common kernel, moving base
    "wb-generic-h64": dict(model="wholebody", H=64, f64=False, generic=True, fast=0),
    "tt64-h32": dict(model="arm", H=32, f64=True, track=True),          # k_rollout_tt
}
B_FORMS = ("arm64-h32", "arm32-h32", "generic64-h32", "generic32-h32", "wb-h64", "tt64-h32")


def _dump(name, record):
    out_path = os.environ.get("MPPI_ACCURACY_OUT")
    print(name, json.dumps(record))
    if out_path:
        with open(out_path.replace(".json", f"_envelope_{name}.json"), "w") as f:
            json.dump({"test": name, "record": record}, f, indent=1)


class Form:
    def __init__(self, name, monkeypatch):
        f = FORMS[name]
        self.name, self.model, self.H, self.f64 = name, f["model"], f["H"], f["f64"]
        self.generic, self.track, self.full = f.get("generic", False), f.get("track", False), f.get("full", False)
        self.A = 7 if self.model == "arm" else 10
        self.chain = P.GENERIC_CHAIN if self.generic else P.kinova_chain()
        if f.get("env"):
            monkeypatch.setenv("MPPI_NO_KINOVA_PATH", "1")
        self.kw = dict(model=self.model, n_samples=P.K, n_horizon=self.H, noise="injected",
                       chain=self.chain if self.generic else None, cost_terms=("target_track",) if self.track else 0)
        if self.model == "arm":
            self.kw["state_f64"] = self.f64
        # the FK path this configuration takes, from the layout words: the test cannot silently run another
        assert P.chain_fast(**self.kw) == f.get("fast", 2), name

    def engine(self, w):
        from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
        return Engine(make_config(device=0, weights=w, **self.kw))

    def runs(self):
        return [(1.0, 0), (1.0, 1), (1.0, 2), (1.0, 3), (8.0, 2)] if self.full else [(1.0, 0), (1.0, 2)]

    def start(self):
        return P.HOME if self.model == "arm" else np.concatenate([P.WB_X0, P.HOME])

    def ends(self, scale=1.0):
        q = P.q_ends(scale, self.generic)
        return q if self.model == "arm" else P.wb_ends(q)

    def state(self, base):
        return P.arm_state(base) if self.model == "arm" else P.wb_state(base[3:])

    def step(self, e, base, noise, tpos, tquat):
        """One control step from rest on `noise`; (trajectory (K, H, C), S (K))."""
        if self.track:
            e.set_target(P.TPOS, P.TQUAT)
            e.set_target_trajectory(tpos, tquat)
        else:
            e.set_target(tpos, tquat)
        e.set_u_prev(np.zeros((self.H, self.A), np.float32))
        e.step(self.state(base), noise[None])
        return e.get_trajectory()[0], e.get_costs()[0]

    def exact(self, base, noise, u_prev=None):
        if self.model == "arm":
            return P.exact_arm(self.chain, base, noise, u_prev)
        return P.exact_wb(self.chain, base[3:], noise, u_prev)

    def exact_fk(self, base, pos):
        if self.model == "arm":
            return P.exact_arm_fk(self.chain, base, pos)
        return P.exact_wb_fk(self.chain, base[3:], pos)

    def stage_a(self, base, tr, what, noise=None, u_prev=None, quiet=False, wound=False):
        """The stored positions against the exact integration, the stored EE against the exact FK:
        of the float64 step (fp64 state), of the stored positions themselves (fp32 state).  Returns
        the exact EE of the float64 step and the achieved maxima."""
        A = self.A
        tr = tr if tr.ndim == 3 else tr[None]   # (the plan: one trajectory)
        pos = tr[..., :A]
        pos_x, ee_x = self.exact(base, noise, u_prev)
        ee_ref = ee_x if self.f64 else self.exact_fk(base, pos.astype(np.float64))
        ee_got = tr[..., A:].reshape(pos.shape[:2] + (16,))
        q_err = np.abs(pos[..., A - 7:] - pos_x[..., A - 7:])
        # (the whole-body state wound up to 48 rad: the integrator's worst-case rounding, P.q_rounding_bound)
        rounding = wound and self.model == "wholebody"
        q_lim = (P.q_rounding_bound if rounding else P.q_tol)(pos_x[..., A - 7:], P.HOME)
        rec = {"q_err": float(q_err.max()),
               "q_err_over_tol": float((q_err / P.q_tol(pos_x[..., A - 7:], P.HOME)).max()),
               "q_err_over_bound": float((q_err / q_lim).max()),
               "ee_err": float(np.abs(ee_got.astype(np.float64) - ee_ref.reshape(ee_got.shape)).max())}
        if not quiet:
            print(f"{what}: stage A {rec}")
        if A == 10:
            P.assert_none(np.abs(pos[..., :3] - pos_x[..., :3]) > P.TOL_X, what + ": base positions")
        P.assert_none(P.q_bad(pos[..., A - 7:], pos_x[..., A - 7:], P.HOME, rounding_bound=rounding),
                      what + ": stored joint angles")
        P.assert_none(P.fk_bad(ee_got, ee_ref), what + ": EE against the exact FK")
        return ee_x, rec

    def oracle(self, base, noise, tpos, tquat, w, u_prev=None):
        """The fp32 oracle's step: (S (K), EE (K, H, 4, 4))."""
        if self.model == "arm":
            r = P.oracle_arm(self.chain, base, noise, np.reshape(tpos, (-1, 3))[0], np.reshape(tquat, (-1, 4))[0], w,
                             self.f64, u_prev)
        else:
            r = P.oracle_wb(self.chain, base[3:], noise, tpos, tquat, w, u_prev)
        if self.track:
            return TO.pose_cost_tracking(r["ee"], tpos, tquat, P.weights_of(w)).numpy(), r["ee"]
        return r["S"].numpy(), r["ee"]


def _rel(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.abs(want)))


# ------------------------------------------------------------------ stages A and C, every form
@pytest.mark.parametrize("name", list(FORMS))
def test_fk_and_cost_sum(name, monkeypatch):
    f = Form(name, monkeypatch)
    engines = {w: f.engine(w) for w in (P.DEFAULT_W, P.OTHER_W)}
    record = {}
    try:
        for scale, b in f.runs():
            base = BASES[b]
            noise = P.ray_noise(f.ends(scale), f.start(), f.H)
            tgt = (np.asarray(P.TPOS, np.float32), np.asarray(P.TQUAT, np.float32))
            for w, e in engines.items():
                what = f"{name} scale {scale:g} base {b} weights {w}"
                if f.track and w is P.DEFAULT_W:   # (the table's targets are built on this run's exact pose)
                    ee5 = f.exact(base, noise)[1][P.K_STAR, -1]
                    tgt = P.target_table(P.target_cases(ee5), f.H)
                tr, S = f.step(e, base, noise, *tgt)
                assert np.isfinite(S).all() and np.isfinite(tr).all(), what
                rec = record.setdefault(f"scale{scale:g}-base{b}", {})
                if w is P.DEFAULT_W:
                    rec.update(f.stage_a(base, tr, what, noise, wound=scale > 1.0)[1])
                S_ref = f.oracle(base, noise, tgt[0], tgt[1], w)[0]
                rec[f"S_rel_{'default' if w is P.DEFAULT_W else 'other'}"] = _rel(S, S_ref)
                print(f"{what}: stage C max rel {_rel(S, S_ref):.2e}")
                P.assert_none(P.S_bad(S, S_ref), what + ": S against the oracle")
    finally:
        for e in engines.values():
            e.close()
        _dump(f"ac_{name}", record)


# ----------------------------------------------------------------------- stage B: the targets
def _stage_b(f, singular):
    """The orientation norm and the position norm alone, per target case and posture set."""
    base = BASES[2]
    e_ori, e_pos = f.engine(P.ORI_ONLY), f.engine(P.POS_ONLY)
    record, bad_cases = {}, []
    try:
        ends = f.ends()
        cl = P.cluster_ends(ends[:, f.A - 7:])
        sets = {"ray": ends, "cluster": cl if f.A == 7 else np.concatenate([np.tile(ends[P.K_STAR, :3], (P.K, 1)), cl], 1)}
        ee5 = f.exact(base, P.ray_noise(ends, f.start(), f.H))[1][P.K_STAR, -1]
        cases = P.singular_cases(ee5) if singular else P.target_cases(ee5)
        for pset, e_nd in sets.items():
            noise = P.ray_noise(e_nd, f.start(), f.H)
            for i, (cname, tp, tq) in enumerate(cases):
                what = f"{f.name} {pset} {cname}"
                tgt = (tp, tq)
                if f.track:   # the case on the terminal row, the others cycling above it
                    tgt = P.target_table(cases, f.H, shift=(i - (f.H - 1)) % len(cases))
                tR = P.target_rotation(tq)
                tr, S = f.step(e_ori, base, noise, *tgt)
                ee_term = tr[:, -1, f.A:].reshape(P.K, 4, 4)
                bad, err, cp = P.ori_bad(S, ee_term, tR)
                rec = {"ori_err": float(err.max()), "ori_err_over_atol": float((err / P.ori_atol(cp)).max()),
                       "ori_err_cos_pitch": float((err * cp).max()), "min_cos_pitch": float(cp.min())}
                if singular:
                    assert np.isfinite(S).all(), what
                    # (yaw and roll reach fl32(pi) > pi: the bound in float32, two ulp for the squares and the root)
                    assert S.max() <= P.ORI_MAX * (1.0 + 2.0 ** -22), (what, float(S.max()))
                    bad = bad & (cp >= P.MIN_COS_PITCH)
                    rec["compared"] = int((cp >= P.MIN_COS_PITCH).sum())
                    rec["ori_err_over_atol"] = float((err / P.ori_atol(cp))[cp >= P.MIN_COS_PITCH].max(initial=0.0))
                else:
                    assert cp.min() >= P.MIN_COS_PITCH, what
                    tr, S = f.step(e_pos, base, noise, *tgt)
                    ee_term = tr[:, -1, f.A:].reshape(P.K, 4, 4)
                    pbad, perr = P.posnorm_bad(S, ee_term, tp)
                    rec["pos_err"] = float(perr.max())
                    if pbad.any():
                        bad_cases.append(f"{what}: position norm, {int(pbad.sum())} samples, max err {perr.max():.2e}")
                record[f"{pset}/{cname}"] = rec
                print(what, rec)
                if bad.any():
                    bad_cases.append(f"{what}: orientation norm, {int(bad.sum())} samples, max err / atol "
                                     f"{(err / P.ori_atol(cp))[bad].max():.2f}")
    finally:
        e_ori.close()
        e_pos.close()
        summary = {k: max(r.get(k, 0.0) for r in record.values())
                   for k in ("ori_err_over_atol", "ori_err_cos_pitch", "pos_err")}
        _dump(f"b_{'singular_' if singular else ''}{f.name}", {"max": summary, "cases": record})
    assert not bad_cases, "\n".join(bad_cases)


@pytest.mark.parametrize("name", B_FORMS)
def test_cost_functions_over_the_targets(name, monkeypatch):
    _stage_b(Form(name, monkeypatch), singular=False)


@pytest.mark.parametrize("name", B_FORMS)
def test_cost_functions_at_the_singularity(name, monkeypatch):
    """Error rotations 1e-4 from and on the gimbal singularity: every cost finite and at most
    sqrt(pi^2 + (pi/2)^2 + pi^2); the samples with cos(pitch) >= 1e-4 within the tolerance.  The
    reference is discontinuous there, so no value is asserted for the rest."""
    _stage_b(Form(name, monkeypatch), singular=True)


# ----------------------------------------------------------------------------- the plan kernel
@pytest.mark.parametrize("name", ["arm64-h32", "arm32-h32", "generic64-h32", "generic32-h32", "wb-h64", "wb-generic-h64"])
def test_plan_fk_and_cost(name, monkeypatch):
    """k_plan: one ray through u_prev row 0 per call, 17 of the 256 rays, bases 0 and 2: the stored
    rows (stage A), cost_t and S (stage C) under both sets of weights."""
    f = Form(name, monkeypatch)
    lanes = sorted(set(range(0, P.K, 16)) | {P.K_STAR})
    engines = {w: f.engine(w) for w in (P.DEFAULT_W, P.OTHER_W)}
    zero = np.zeros((1, f.H, f.A), np.float32)
    worst = {"ee_err": 0.0, "S_rel": 0.0, "cost_t_err_over_S": 0.0}
    try:
        for b in (0, 2):
            base = BASES[b]
            rows = P.ray_rows(f.ends(), f.start(), f.H)
            for k in lanes:
                u = np.zeros((f.H, f.A), np.float32)
                u[0] = rows[k]
                for w, e in engines.items():
                    what = f"{name} plan base {b} ray {k} weights {w}"
                    e.set_target(P.TPOS, P.TQUAT)
                    e.set_u_prev(u)
                    e.set_state(f.state(base))
                    p = e.get_plan().vehicle(0)
                    if w is P.DEFAULT_W:
                        rec = f.stage_a(base, p.traj, what, zero, u, quiet=True)[1]
                        worst["ee_err"] = max(worst["ee_err"], rec["ee_err"])
                    S_ref, ee = f.oracle(base, zero, P.TPOS, P.TQUAT, w, u)
                    c_ref = P.oracle_cost_t(ee[0], P.TPOS, P.TQUAT, w)
                    worst["S_rel"] = max(worst["S_rel"], _rel(p.S, S_ref[0]))
                    worst["cost_t_err_over_S"] = max(worst["cost_t_err_over_S"],
                                                     float(np.abs(p.cost_t - c_ref).max() / S_ref[0]))
                    P.assert_none(P.S_bad([p.S], S_ref), what + ": S")
                    P.assert_none(np.abs(p.cost_t - c_ref) > P.TOL_S * abs(S_ref[0]), what + ": cost_t")
    finally:
        for e in engines.values():
            e.close()
        _dump(f"plan_{name}", worst)


# ------------------------------------------------------- the base quaternion off the unit sphere
def test_base_quaternion_off_the_unit_sphere(monkeypatch):
    """Base 2's quaternion times 1 + eps (1e-6: a unit quaternion carried in float32).  The oracle does
    not normalise it either (stage A unchanged), but inverts the EE rotation where pose_cost takes the
    transpose: S at 2e-5 relative up to eps = 1e-6; eps = 1e-4 is recorded, not asserted."""
    f = Form("arm64-h32", monkeypatch)
    e = f.engine(P.DEFAULT_W)
    noise = P.ray_noise(f.ends(), f.start(), f.H)
    record = {}
    try:
        for eps in (0.0, 3e-8, 1e-6, 1e-4):
            base = BASES[2].copy()
            base[3:] *= 1.0 + eps
            what = f"base quaternion x (1 + {eps:g})"
            tr, S = f.step(e, base, noise, P.TPOS, P.TQUAT)
            S_ref = f.oracle(base, noise, P.TPOS, P.TQUAT, P.DEFAULT_W)[0]
            ee_x = f.exact(base, noise)[1]
            record[f"{eps:g}"] = {"S_rel": _rel(S, S_ref),
                                  "ee_err": float(np.abs(tr[..., 7:].reshape(ee_x.shape) - ee_x).max())}
            print(what, record[f"{eps:g}"])
            if eps <= 1e-6:
                f.stage_a(base, tr, what, noise)
                P.assert_none(P.S_bad(S, S_ref), what + ": S against the oracle (true inverse)")
    finally:
        e.close()
        _dump("base_quaternion", record)
