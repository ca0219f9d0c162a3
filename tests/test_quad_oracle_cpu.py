"""tests/quad_oracle.py checked on the CPU: the float64 rollout against an independent longdouble restatement,
against the torch oracle in float64 and against closed-form motions; the closed-form inv(J); the fp32 restatement
of the kernel's chain inside the bound on every design, in both modes, with and without sin/cos noise; every
planted mistake outside the bound in the quantity named for it; and the shares the validity and circular rules
set aside, for the inputs of every case tests/test_gpu_quad_envelope.py flies.  No GPU calls.
With QUAD_ENVELOPE_LOG set every err / bound is appended to that file (profiles/r20/quad_envelope)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import quad_oracle as Q
from oracle import mppi_oracle as O

K, H = 100, 64
MODES = (False, True)


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("QUAD_ENVELOPE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _scale_close(a, b, mask, what, rel=1e-12):
    for name, x, y in zip(("pos", "ang", "vel", "rate"), a, b):
        x, y = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
        d = np.abs(x - y)
        if name == "ang":   # (the wrap's branch at +-pi itself: either is right)
            d = np.minimum(d, np.abs(2 * math.pi - d))
        err = float(np.max(np.where(mask[..., None], d, 0)))
        scale = float(np.max(np.abs(np.where(mask[..., None], y, 0))))
        assert err <= rel * max(scale, 1.0), (what, name, err, scale)


@pytest.mark.parametrize("literal", MODES)
def test_rollout_matches_longdouble(literal):
    for d in Q.DESIGNS:
        u, eps = d.inputs(16, H)
        ro = Q.rollout(u, eps, d.x, d.v, d.cfg, literal)
        ref = Q.rollout_values(u, eps, d.x, d.v, d.cfg, literal, np.longdouble)
        _scale_close((ro.pos, ro.ang, ro.vel, ro.rate), ref, ro.valid, d.name)
        ld = Q.rollout(u, eps, d.x, d.v, d.cfg, literal, np.longdouble)   # the bound does not depend on the value's type
        np.testing.assert_allclose(ld.bound_e, ro.bound_e, rtol=1e-9)


@pytest.mark.parametrize("literal", MODES)
def test_rollout_matches_torch_oracle_in_float64(literal):
    for d in Q.DESIGNS:
        u, eps = d.inputs(16, H)
        ro = Q.rollout(u, eps, d.x, d.v, d.cfg, literal)
        dt, im, iinv, kd, g = d.cfg.device()
        P = O.QuadParams(mass=1.0 / im, inertia=tuple(1.0 / i for i in iinv), kd=kd, gravity=g)
        x0 = np.asarray(d.x, np.float32).astype(np.float64)
        v0 = np.asarray(d.v, np.float32).astype(np.float64)
        with O.float64_everywhere():
            tr = O.quad_rollout(torch.from_numpy(u.astype(np.float64) + eps.astype(np.float64)), x0, v0, dt, P, literal).numpy()
        _scale_close((ro.pos, ro.ang), (tr[..., :3], tr[..., 3:]), ro.valid, d.name)


def test_closed_form_inverse():
    for d in Q.DESIGNS:
        u, eps = d.inputs(16, H)
        ro = Q.rollout(u, eps, d.x, d.v, d.cfg, True)
        e = ro.ang[ro.valid]
        err = np.abs(Q.inv_jacobian(e) - np.linalg.inv(Q.jacobian(e))).max()
        assert err <= 1e-12 * max(1.0, np.abs(Q.jacobian(e)).max()), (d.name, err)


# ------------------------------------------------------------- closed-form motions (test_quadrotor_cpu.py's), float64
M, G, DT = Q._f(14.7), Q._f(9.81), Q._f(0.01)


def _fly(u, x, v=(0.0,) * 6):
    u = np.asarray(u, np.float32)
    return Q.rollout(u, np.zeros((1,) + u.shape, np.float32), x, v)


def test_hover_thrust_holds_position():
    u = np.zeros((32, 4))
    u[:, 0] = 1.0 / Q.Cfg().device()[1] * G   # thrust / m = g to an ulp of fp32 (the fp32 thrust is what flies)
    ro = _fly(u, [0.3, -0.2, 1.0, 0, 0, 0.5])
    a = Q.Cfg().device()[1] * float(np.float32(u[0, 0])) - G   # the residual acceleration of the rounded thrust
    t = np.arange(1, 33)
    want_z = np.float64(np.float32(1.0)) + a * DT * DT * (t * (t + 1) / 2 - 1)
    assert np.abs(ro.pos[0, :, 2] - want_z).max() < 1e-13
    assert np.abs(ro.pos[0, :, :2] - np.float32([0.3, -0.2]).astype(np.float64)).max() < 1e-15
    assert np.abs(ro.ang[0, :, 2] - 0.5).max() == 0.0


def test_free_fall_is_semi_implicit_euler():
    """z_t = z0 - g dt^2 sum_{i=1..t} (i+1): step 0 moves with the measured velocity, later steps with the new one."""
    ro = _fly(np.zeros((20, 4)), [0, 0, 5.0, 0, 0, 0])
    want = [5.0 - G * DT * DT * sum(i + 1 for i in range(1, t + 1)) for t in range(20)]
    assert np.abs(ro.pos[0, :, 2] - want).max() < 1e-14


def test_yaw_torque_spins_only_yaw():
    Hh = 16
    u = np.zeros((Hh, 4))
    u[:, 0] = M * G
    u[:, 3] = 2.59
    ro = _fly(u, [0, 0, 1.0, 0, 0, 0])
    a = Q.Cfg().device()[2][2] * float(np.float32(2.59))   # fl32(1 / I_zz) tau
    wz = [DT * a * (t + 1) for t in range(Hh)]
    yaw = [sum(DT * w for w in wz[1:t + 1]) for t in range(Hh)]   # step 0 integrates the measured rate
    assert np.abs(ro.ang[0, :, 2] - yaw).max() < 1e-15
    assert np.abs(ro.rate[0, :, 2] - wz).max() < 1e-15
    assert np.abs(ro.ang[0, :, :2]).max() == 0.0 and np.abs(ro.pos[0, :, :2]).max() == 0.0


def test_tilted_thrust_accelerates_sideways():
    """Roll phi tilts body z toward -y: a_y = -g tan(phi) at the thrust that holds altitude."""
    phi = float(np.float32(0.2))
    u = np.zeros((3, 4))
    u[:, 0] = M * G / math.cos(phi)
    ro = _fly(u, [0, 0, 1.0, phi, 0, 0])
    thr = float(np.float32(u[0, 0]))
    ay = -Q.Cfg().device()[1] * thr * math.sin(phi)
    assert abs((ro.pos[0, 1, 1] - ro.pos[0, 0, 1]) / DT - 2 * ay * DT) < 1e-13
    assert abs(ay + G * math.tan(phi)) < 1e-5 and abs(ro.pos[0, 2, 2] - 1.0) < 1e-6


# --------------------------------------------------------------------------------- the bound: inside, and outside
def _ratios(d, literal, mistake=None, noisy=False, Kk=K, Hh=H):
    u, eps = d.inputs(Kk, Hh)
    ro = Q.rollout(u, eps, d.x, d.v, d.cfg, literal)
    em = Q.emulate(u, eps, d.x, d.v, d.cfg, literal, d.target, mistake=mistake,
                   noise_rng=np.random.default_rng(5) if noisy else None)
    return ro, Q.compare(ro, em["traj"], em["S"], d.target)


@pytest.mark.parametrize("design", Q.DESIGNS, ids=[d.name for d in Q.DESIGNS])
def test_emulation_inside_the_bound(design):
    for literal in MODES:
        for noisy in (False, True):
            ro, r = _ratios(design, literal, noisy=noisy)
            _log(dict(side="cpu", case=f"{design.name}-{'lit' if literal else 'J'}", sincos_noise=noisy,
                      pos=round(r.pos, 4), ang=round(r.ang, 4), S=round(r.S, 4), excluded=r.excluded, circular=r.circular,
                      bound_p=float(np.where(ro.valid[..., None], ro.bound_p, 0).max()),
                      bound_e=float(np.where(ro.valid[..., None], ro.bound_e, 0).max())))
            assert max(r.pos, r.ang, r.S) <= 1.0, (design.name, literal, noisy, r)
            assert r.excluded <= Q.EXCLUDED_CAP and r.circular <= Q.CIRCULAR_CAP, (design.name, literal, r)


def test_every_mistake_is_named_by_a_design():
    named = {m for d in Q.DESIGNS for lit in MODES for m in Q.exposes(d, lit)}
    assert named == set(Q.MISTAKES), set(Q.MISTAKES) - named


@pytest.mark.parametrize("design", Q.DESIGNS, ids=[d.name for d in Q.DESIGNS])
def test_planted_mistakes_outside_the_bound(design):
    for literal in MODES:
        for m in Q.exposes(design, literal):
            _, r = _ratios(design, literal, mistake=m)
            _log(dict(side="cpu", case=f"{design.name}-{'lit' if literal else 'J'}", mistake=m, shows_in=Q.SHOWS_IN[m],
                      ratio=float(f"{Q.exposed(r, m):.4g}")))
            assert Q.exposed(r, m) > 1.0, (design.name, literal, m, r)


def test_first_step_outputs_bound_holds_for_an_fp32_restatement():
    """quad_outputs restated in numpy float32 stays inside first_step_outputs' bound on every design; a step-0
    mistake (the updated rates) does not."""
    f = np.float32
    for d in Q.DESIGNS:
        dt, im, iinv, kd, g = (f(c) if np.isscalar(c) else np.asarray(c, f) for c in d.cfg.device())
        x, v = np.asarray(d.x, f), np.asarray(d.v, f)
        u0 = d.inputs(1, 3)[0][0]
        sr, sp, sy = np.sin(x[3:]).astype(f)
        cr, cp, cy = np.cos(x[3:]).astype(f)
        tp = sp / cp
        r = np.array([cy * sp * cr + sy * sr, sy * sp * cr - cy * sr, cp * cr], f)
        w = v[3:]
        de = np.array([w[0] + sr * tp * w[1] + cr * tp * w[2], cr * w[1] - sr * w[2], sr / cp * w[1] + cr / cp * w[2]], f)
        gv = np.array([0, 0, -g], f)
        nv = v[:3] + dt * (gv + im * (r * u0[0] - kd * v[:3]))
        nw = w + dt * (iinv * u0[1:])
        got = np.concatenate([x[:3] + dt * v[:3], x[3:] + dt * de, nv, nw]).astype(np.float64)
        want, b = Q.first_step_outputs(d.x, d.v, u0, d.cfg)
        assert (np.abs(got - want) <= b).all(), (d.name, np.abs(got - want) / b)
        bad = (x[3:] + dt * np.array([nw[0] + sr * tp * nw[1] + cr * tp * nw[2], cr * nw[1] - sr * nw[2],
                                      sr / cp * nw[1] + cr / cp * nw[2]], f)).astype(np.float64)
        assert (np.abs(bad - want[3:6]) > b[3:6]).any(), d.name


# ------------------------------------------------------------------------ the GPU cases' inputs: both caps, on the CPU
ALL_CASES = Q.DYNAMICS + Q.LOOPS + Q.BLOCKS + Q.TRACK


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.tag for c in ALL_CASES])
def test_gpu_case_inputs_meet_the_caps(case):
    """From the reference arithmetic alone, and for the fp32 restatement: samples the validity rule drops <= 2%,
    angle elements compared modulo 2 pi <= 1%, per vehicle."""
    for v, (d, u, eps, tg) in enumerate(case.vehicles()):
        ro = Q.rollout(u, eps, d.x, d.v, d.cfg, case.literal)
        em = Q.emulate(u, eps, d.x, d.v, d.cfg, case.literal, tg)
        r = Q.compare(ro, em["traj"], em["S"], tg)
        assert r.excluded <= Q.EXCLUDED_CAP and r.circular <= Q.CIRCULAR_CAP, (case.tag, v, d.name, r.excluded, r.circular)
        assert max(r.pos, r.ang, r.S) <= 1.0, (case.tag, v, d.name, r)
        if v == 0:   # the discrimination the GPU case asserts first
            for m in Q.exposes(d, case.literal):
                bad = Q.emulate(u, eps, d.x, d.v, d.cfg, case.literal, tg, mistake=m)
                assert Q.exposed(Q.compare(ro, bad["traj"], bad["S"], tg), m) > 1.0, (case.tag, m)


@pytest.mark.parametrize("name,Hh,literal", Q.PLAN, ids=[f"{n}-H{h}-{Q._mode(lit)}" for n, h, lit in Q.PLAN])
def test_plan_case_inputs(name, Hh, literal):
    """The plan cases' zero-noise sample: valid throughout, the fp32 restatement inside the bound, the two named
    mistakes outside."""
    d = Q.BY_NAME[name]
    u, _ = d.inputs(1, Hh)
    zero = np.zeros((1, Hh, 4), np.float32)
    ro = Q.rollout(u, zero, d.x, d.v, d.cfg, literal)
    assert ro.valid.all()
    em = Q.emulate(u, zero, d.x, d.v, d.cfg, literal, d.target)
    r = Q.compare(ro, em["traj"], em["S"], d.target)
    assert max(r.pos, r.ang, r.S) <= 1.0, r
    for m in Q.plan_exposes(d, literal):
        bad = Q.emulate(u, zero, d.x, d.v, d.cfg, literal, d.target, mistake=m)
        assert Q.exposed(Q.compare(ro, bad["traj"], bad["S"], d.target), m) > 1.0, (name, Hh, literal, m)


def test_circular_rule_at_the_wrap():
    """A pre-wrap value within its bound of an odd multiple of pi is compared modulo 2 pi (either branch of rint is
    right there); one clear of it is compared as stored, so a missing wrap still fails."""
    b = np.zeros((3, Q.NT))
    b[:, 0] = 1e-7
    x = Q._B(np.array([math.pi + 5e-8, -3 * math.pi - 5e-8, math.pi + 1e-3]), b)
    wrapped, circ = Q._wrap(x)
    assert circ.tolist() == [True, True, False]
    assert np.abs(np.abs(wrapped.v[:2]) - math.pi).max() < 1e-7 and abs(wrapped.v[2] - (1e-3 - math.pi)) < 1e-12
    d = Q.BY_NAME["yaw_wrap"]
    u, eps = d.inputs(4, 8)
    ro = Q.rollout(u, eps, d.x, d.v, d.cfg)
    t = int(np.argmax(np.abs(np.diff(ro.ang[0, :, 2])) > 6.0)) + 1      # the step whose yaw wrapped
    other = np.concatenate([ro.pos, ro.ang], -1)
    other[0, t, 5] += 2 * math.pi                                      # the other branch, stored
    assert Q.compare(ro, other).ang > 1.0
    ro.circ[0, t, 2] = True
    assert Q.compare(ro, other).ang <= 1.0
