"""Value-function clipping (PPO2's cliprange_vf): ppo_set_value_clip / ppo_get_value_clip, PPOHip.set_value_clip, the host layer's cliprange_vf.

PPO_VCLIP_POLICY (the default) clips the value with cliprange, PPO_VCLIP_RANGE with its own range, PPO_VCLIP_OFF not at all.  The two towers are separate
networks, so the reference of a RANGE step is spliced from two oracle calls: the policy entries and losses 0, 2, 3, 4 from loss_grad(cliprange=cr), the value
entries and loss 1 from loss_grad(cliprange=r).  OFF takes the value tower from a float64 torch evaluation of (v - R)^2.  Then clip + Adam as Oracle.train_step.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as o
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CR = 0.16102319955825806
LR = 0.000393141177482903
R_VF = 0.05                  # a value-clip range well inside cr: rows with |v - vo| between the two change branch
POLICY, RANGE, OFF = 0, 1, 2


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def vf_mask(tensors, P):
    """True on the value tower's entries (vf_fc*/*, vf/*) of a dense flat vector"""
    m = np.zeros(P, bool)
    off = 0
    for name, shape in tensors:
        cnt = int(np.prod(shape))
        if name.startswith("vf"):
            m[off:off + cnt] = True
        off += cnt
    return m


def oracle_tensors(orc):
    return [(n, shape) for n, _, shape in orc.tensors]


def clear_value_edges(v, old_v, ret, ranges):
    """Moves rows off the value loss's discontinuities for every clip range in `ranges` (|v - vo| == r, and (v-R)^2 == (vclip-R)^2 where the clip
    is active): within ~1e-5 of one, the side a row falls on is decided by the summation order (tests/helpers.synth_minibatch)."""
    v = v.astype(np.float64)
    for _ in range(3):
        for r in ranges:
            dvo = v - old_v
            near = np.abs(np.abs(dvo) - r) < 1e-3
            old_v[near] -= np.float32(0.004) * np.sign(dvo[near]).astype(np.float32)
            dvo = v - old_v
            vclip = old_v + np.clip(dvo, -r, r)
            s1, s2 = (v - ret) ** 2, (vclip - ret) ** 2
            near = (np.abs(dvo) > r) & (np.abs(s1 - s2) < 1e-3 * np.maximum(s1, 1e-6))
            ret[near] += np.float32(0.05)
    return old_v, ret


def gaussian_batch(orc, n, seed):
    mb = H.synth_minibatch(orc, n, seed)
    v = orc.forward(mb["obs"])[1]
    old_v, ret = clear_value_edges(v, mb["old_values"].copy(), mb["returns"].copy(), (CR, R_VF))
    dvo = np.abs(v.astype(np.float64) - old_v)
    assert np.mean((dvo > R_VF) & (dvo < CR)) > 0.15                          # a good share of rows lies between the two ranges
    return (mb["obs"], mb["actions"], o.adv_normalize(ret, old_v), ret, mb["old_neglogp"], old_v)


def torch_value_off(theta, tensors, hidden, obs, returns, vf_coef):
    """(vf_loss, gradient of vf_coef * vf_loss) for the unclipped 0.5 mean (v - R)^2: torch float64 autograd over the value tower"""
    import torch
    d = torch.float64
    th = torch.tensor(np.asarray(theta, np.float64), requires_grad=True)
    offs, off = {}, 0
    for name, shape in tensors:
        offs[name] = (off, shape); off += int(np.prod(shape))

    def T(name):
        a, shape = offs[name]
        return th[a:a + int(np.prod(shape))].reshape(shape)
    h = torch.tensor(np.asarray(obs, np.float64))
    for l in range(len(hidden)):
        h = torch.tanh(h @ T("vf_fc%d/w" % l) + T("vf_fc%d/b" % l))
    v = (h @ T("vf/w")).reshape(-1) + T("vf/b")[0]
    vf_loss = 0.5 * ((v - torch.tensor(np.asarray(returns, np.float64))) ** 2).mean()
    (vf_coef * vf_loss).backward()
    return vf_loss.item(), th.grad.numpy().copy()


def spliced_loss_grad(orc, args, cr, mode, r):
    """the reference's (losses, pre-clip gradient) of one train step of the Gaussian head under a value-clip setting"""
    lp, gp = orc.loss_grad(*args, cr)
    if mode == POLICY:
        return lp, gp
    m = vf_mask(oracle_tensors(orc), orc.P)
    if mode == RANGE:
        lv, gv = orc.loss_grad(*args, r)
        vf = lv[1]
    else:
        vf, gv = torch_value_off(orc.theta, oracle_tensors(orc), orc.hidden, args[0], args[3], orc.cfg.vf_coef)
    losses, grad = lp.copy(), gp.copy()
    losses[1] = vf
    grad[m] = gv[m]
    return losses, grad


def spliced_train_step(orc, args, lr, cr, mode, r):
    losses, grad = spliced_loss_grad(orc, args, cr, mode, r)
    g, _ = orc.clip(grad)
    orc.adam(g, lr)
    return losses, grad


def new_oracle(hidden, O=18, A=18, seed=3):
    orc = o.Oracle(O, A, list(hidden))
    orc.init_orthogonal(seed)
    orc.tensor("pi/logstd")[:] = np.random.RandomState(seed + 1).uniform(-1.0, 0.2, (1, A))
    return orc


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_library_exports_them():
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    for name, val in (("PPO_VCLIP_POLICY", 0), ("PPO_VCLIP_RANGE", 1), ("PPO_VCLIP_OFF", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"int ppo_set_value_clip\(ppo_handle\* h, int32_t mode, float range\);", hdr)
    assert re.search(r"int ppo_get_value_clip\(const ppo_handle\* h, int32_t\* mode, float\* range\);", hdr)
    assert re.search(r"#define PPO_ABI_VERSION 3\b", hdr)
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library(build=False)
    assert lib.ppo_abi_version() == 3
    assert hasattr(lib, "ppo_set_value_clip") and hasattr(lib, "ppo_get_value_clip")
    import ctypes
    assert lib.ppo_set_value_clip(None, RANGE, ctypes.c_float(0.1)) != 0      # a null handle is an error, not a crash
    assert b"null" in lib.ppo_last_error(None)


def test_spliced_reference_is_consistent():
    orc = new_oracle((64, 64))
    args = gaussian_batch(orc, 256, 11)
    plain_l, plain_g = orc.loss_grad(*args, CR)
    same_l, same_g = spliced_loss_grad(orc, args, CR, RANGE, CR)
    np.testing.assert_array_equal(same_l, plain_l)
    np.testing.assert_array_equal(same_g, plain_g)
    m = vf_mask(oracle_tensors(orc), orc.P)
    for mode in (RANGE, OFF):
        l, g = spliced_loss_grad(orc, args, CR, mode, R_VF)
        np.testing.assert_array_equal(l[[0, 2, 3, 4]], plain_l[[0, 2, 3, 4]])
        np.testing.assert_array_equal(g[~m], plain_g[~m])
        assert l[1] != plain_l[1], mode
        assert np.abs(g[m] - plain_g[m]).max() > 1e-3 * np.abs(plain_g[m]).max(), mode
    # the float64 (v - R)^2 against the oracle with an infinite range (vclip = v up to rounding)
    off_l, off_g = spliced_loss_grad(orc, args, CR, OFF, 0.0)
    inf_l, inf_g = spliced_loss_grad(orc, args, CR, RANGE, np.inf)
    close(off_l, inf_l, rtol=1e-5, atol=1e-7)
    close(off_g, inf_g, rtol=2e-4, atol=2e-6 * float(np.abs(inf_g).max()))


def test_mirrored_update_is_oracle_update():
    """the Python restatement of Oracle.update that test_update_matches_spliced_reference drives is Oracle.update itself in POLICY mode"""
    E, T, nmb = 4, 16, 2
    a, b = new_oracle((16, 8)), new_oracle((16, 8))
    ro = rollout_inputs(a, E, T)
    rng = np.random.RandomState(8)
    perms = np.stack([rng.permutation(E * T).astype(np.int32) for _ in range(2)])
    rows_ref, _ = a.update(ro, perms, nmb, LR, CR)
    rows = mirrored_update(b, ro, perms, nmb, LR, CR, POLICY, 0.0)
    close(rows, rows_ref, rtol=1e-6, atol=1e-9)
    close(b.theta, a.theta, rtol=1e-6, atol=1e-9)


def test_host_layer_maps_cliprange_vf():
    src = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo2", "ppo2.hpp")).read()
    assert "apply_value_clip();" in src and "ppo_set_value_clip(h_, PPO_VCLIP_OFF" in src
    out = subprocess.run([os.path.join(ROOT, "ppo_cpp_amd", "ppo_cpp_hip"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--cliprange_vf" in out.stdout
    bad = subprocess.run([os.path.join(ROOT, "ppo_cpp_amd", "ppo_cpp_hip"), "--cliprange_vf", "bogus"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--cliprange_vf" in bad.stderr


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
FAMILIES = {                  # name: (hidden, O, A, rows, action_dist, compute_dtype, kernel_counts key)
    "narrow": ((64, 64), 18, 18, 256, "gaussian", 0, "narrow_train_kernel<static>"),
    "train8": ((256, 256), 18, 18, 512, "gaussian", 0, "train8_kernel"),
    "generic": ((128, 96), 18, 18, 256, "gaussian", 0, "train_fwd_bwd_kernel"),
    "categorical": ((64, 64), 18, 6, 256, "categorical", 0, "train_fwd_bwd_kernel<cat>"),
    "bf16": ((256, 256), 18, 18, 256, "gaussian", 1, "bf16_train_sequence"),
}


def categorical_ref(hidden, O, A, seed=9):
    from tests.categorical_ref import CatRef
    ref = CatRef(O, A, hidden)
    ref.init_random(seed)
    return ref


def categorical_batch(ref, n, seed):
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O)).astype(np.float32)
    a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)))
    old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
    ratio = np.exp(old_nlp.astype(np.float64) - nlp)
    near = np.abs(np.abs(ratio - 1.0) - CR) < 1e-3
    old_nlp[near] += np.float32(0.01)
    old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
    ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
    old_v, ret = clear_value_edges(v, old_v, ret, (CR, R_VF))
    return obs, a.astype(np.float32), o.adv_normalize(ret, old_v), ret, old_nlp, old_v


def family_setup(fam, seed=3):
    """(reference or None, initial weights, minibatch, handle factory)"""
    import ppo_cpp_amd
    hidden, O, A, n, dist, dtype, _ = FAMILIES[fam]
    if dist == "categorical":
        ref = categorical_ref(hidden, O, A)
        theta, batch = ref.theta.astype(np.float32), categorical_batch(ref, n, 21)
    else:
        ref = new_oracle(hidden, O, A, seed)
        theta, batch = ref.theta.copy(), gaussian_batch(ref, n, 21)

    def make(compute_dtype=dtype):
        g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist=dist, compute_dtype=compute_dtype)
        g.set_flat(theta)
        return g
    return ref, theta, batch, make


def one_step(make, batch, settings, compute_dtype=None):
    """a fresh handle, the given set_value_clip calls, one train step: (losses, pre-clip gradient, weights)"""
    g = make() if compute_dtype is None else make(compute_dtype)
    for s in settings:
        g.set_value_clip(*s)
    losses = g.train_step(LR, CR, *batch)
    grad, _ = g.last_grad()
    out = (losses, grad, g.get_flat(0), g.kernel_counts())
    g.close()
    return out


@pytest.mark.gpu
def test_errors_and_round_trip():
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
    assert g.get_value_clip() == ("policy", 0.0)
    g.set_value_clip("range", 0.25)
    assert g.get_value_clip() == ("range", pytest.approx(0.25))
    for mode, r in ((3, 0.1), (-1, 0.1), ("range", -0.1), ("range", float("nan")), ("range", float("inf")), (RANGE, float("-inf"))):
        with pytest.raises(ppo_cpp_amd.PPOHipError):
            g.set_value_clip(mode, r)
        assert g.get_value_clip() == ("range", pytest.approx(0.25)), (mode, r)      # a failed set leaves the previous setting
    with pytest.raises(ValueError):
        g.set_value_clip("clip", 0.1)
    g.set_value_clip(OFF, float("nan"))                                      # range is ignored outside RANGE
    assert g.get_value_clip() == ("off", 0.0)
    g.set_value_clip("policy", -5.0)
    assert g.get_value_clip() == ("policy", 0.0)
    g.set_value_clip(RANGE, 0.0)
    assert g.get_value_clip() == ("range", 0.0)
    assert np.frombuffer(g.debug_buffer("hyper").tobytes(), np.uint32).size == 2
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["narrow", "train8", "generic", "categorical"])
def test_train_step_matches_spliced_reference(fam):
    ref, theta, batch, make = family_setup(fam)
    n = batch[0].shape[0]
    for mode, r in ((RANGE, R_VF), (OFF, 0.0)):
        losses, grad, th, kc = one_step(make, batch, [(mode, r)])
        assert kc.get(FAMILIES[fam][6], 0) > 0, kc
        if fam == "categorical":
            rr = categorical_ref(FAMILIES[fam][0], FAMILIES[fam][1], FAMILIES[fam][2])
            lp, gp = rr.loss_grad(*batch, CR)
            lv, gv = rr.loss_grad(*batch, r if mode == RANGE else np.inf)
            m = vf_mask(rr.specs, rr.P)
            ref_l, ref_g = lp.copy(), gp.copy()
            ref_l[1], ref_g[m] = lv[1], gv[m]
            rr.clip_adam(ref_g.copy(), LR)
            ref_theta = rr.theta
        else:
            orc = new_oracle(FAMILIES[fam][0])
            np.testing.assert_array_equal(orc.theta, theta)
            ref_l, ref_g = spliced_train_step(orc, batch, LR, CR, mode, r)
            ref_theta = orc.theta
        close(losses[:4], ref_l[:4], rtol=1e-4, atol=1e-6, msg="%s mode %d losses" % (fam, mode))
        assert abs(float(losses[4]) - float(ref_l[4])) <= 1.01 / n
        gs = float(np.abs(ref_g).max())
        close(grad, ref_g, rtol=2e-4, atol=2e-6 * gs, msg="%s mode %d grad" % (fam, mode))
        close(th, ref_theta, rtol=1e-4, atol=2e-6, msg="%s mode %d theta" % (fam, mode))


def cosine(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


@pytest.mark.gpu
def test_bf16_train_step_follows_the_fp32_path():
    _, _, batch, make = family_setup("bf16")
    P = None
    for mode, r in ((RANGE, R_VF), (OFF, 0.0)):
        lb, gb, _, kc = one_step(make, batch, [(mode, r)])
        assert kc.get("bf16_train_sequence", 0) > 0, kc
        lf, gf, _, _ = one_step(make, batch, [(mode, r)], compute_dtype=0)
        lpol, gpol, _, _ = one_step(make, batch, [], compute_dtype=0)
        assert lb[1] == pytest.approx(lf[1], rel=3e-2), "vf_loss"
        assert lb[0] == pytest.approx(lf[0], abs=1e-2)
        if P is None:
            g = make(); tensors = g.tensors; g.close(); P = gf.size
        m = vf_mask(tensors, P)
        # the bf16 value gradient is that of ITS mode: much nearer the fp32 path's same mode than the fp32 path's POLICY
        assert np.linalg.norm(gb[m] - gf[m]) < 0.5 * np.linalg.norm(gb[m] - gpol[m]), mode
        off = 0
        for name, shape in tensors:
            cnt = int(np.prod(shape))
            if name.startswith("vf") and np.linalg.norm(gf[off:off + cnt]) > 1e-3 * np.linalg.norm(gf):
                assert cosine(gb[off:off + cnt], gf[off:off + cnt]) > 0.995, (name, mode)
            off += cnt


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["narrow", "train8", "generic", "categorical", "bf16"])
def test_invariants_bit_for_bit(fam):
    _, _, batch, make = family_setup(fam)
    g = make(); m = vf_mask(g.tensors, g.P); g.close()
    base = one_step(make, batch, [])
    assert base[3].get(FAMILIES[fam][6], 0) > 0, base[3]
    explicit = one_step(make, batch, [("policy",)])
    same = one_step(make, batch, [("range", CR)])
    back = one_step(make, batch, [("range", R_VF), ("policy",)])
    other = one_step(make, batch, [("range", R_VF)])
    for got, what in ((explicit, "explicit policy"), (same, "range == cliprange"), (back, "range, then policy")):
        for a, b in zip(got[:3], base[:3]):
            np.testing.assert_array_equal(a, b, err_msg=what)
    np.testing.assert_array_equal(other[0][[0, 2, 3, 4]], base[0][[0, 2, 3, 4]])
    np.testing.assert_array_equal(other[1][~m], base[1][~m])
    assert other[0][1] != base[0][1]
    assert not np.array_equal(other[1][m], base[1][m])


def rollout_inputs(orc, E, T, seed=5):
    """a [T, E] rollout of the model's own actions, with stored values and neglogp perturbed so that v - vo and the ratio straddle the clip ranges"""
    rng = np.random.RandomState(seed)
    B, O, A = E * T, orc.O, orc.A
    obs = rng.uniform(-1, 1, (B, O)).astype(np.float32)
    act, v, nlp = orc.step(obs, rng.normal(size=(B, A)).astype(np.float32))
    return {"obs": obs.reshape(T, E, O), "actions": act.reshape(T, E, A),
            "values": (v + rng.normal(scale=0.2, size=B)).astype(np.float32).reshape(T, E),
            "neglogp": (nlp + rng.normal(scale=0.15, size=B)).astype(np.float32).reshape(T, E),
            "returns": (v + rng.normal(scale=0.5, size=B)).astype(np.float32).reshape(T, E)}


def mirrored_update(orc, ro, perms, nmb, lr, cr, mode, r):
    """Oracle.update (oracle/ppo_oracle.c orc_update) restated in Python around spliced_train_step: env-major rows, explicit perms,
    per-minibatch advantage normalisation"""
    T, E = ro["values"].shape
    B = E * T
    M = B // nmb
    flat = {k: np.swapaxes(a, 0, 1).reshape((B,) + a.shape[2:]) for k, a in ro.items()}
    rows = []
    for perm in perms:
        inv = np.empty(B, np.int64)
        inv[perm] = np.arange(B)
        for k in range(nmb):
            idx = inv[k * M:(k + 1) * M]
            ret, val = flat["returns"][idx], flat["values"][idx]
            args = (flat["obs"][idx], flat["actions"][idx], o.adv_normalize(ret, val), ret, flat["neglogp"][idx], val)
            rows.append(spliced_train_step(orc, args, lr, cr, mode, r)[0])
    return np.array(rows)


def make_update_handle(hidden, E, T, ro, theta, state=None):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(18, 18, list(hidden))
    g.set_flat(theta)
    if state is not None:
        g.set_flat(state[0], 0); g.set_flat(state[1], 1); g.set_flat(state[2], 2); g.set_beta_powers(state[3])
    g.rollout_alloc(E, T)
    for f, a in ro.items():
        g.rollout_set(f, a)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,E,T,nmb,key", [((256, 256), 16, 64, 4, "train8_kernel"), ((64, 64), 8, 32, 8, "narrow_epoch_kernel")])
def test_graph_replay_follows_the_setting(hidden, E, T, nmb, key):
    """ppo_update captures its launch sequence once and replays it: a setting changed in between must reach the replay"""
    epochs, B = 2, E * T
    orc = new_oracle(hidden)
    ro = rollout_inputs(orc, E, T)
    rng = np.random.RandomState(8)
    perms = np.stack([rng.permutation(B).astype(np.int32) for _ in range(epochs)])
    a = make_update_handle(hidden, E, T, ro, orc.theta)
    a.update(LR, CR, epochs, nmb, perms)                                 # captured under POLICY
    state = (a.get_flat(0), a.get_flat(1), a.get_flat(2), a.beta_powers())
    for mode, r in ((RANGE, R_VF), (OFF, 0.0), (POLICY, 0.0)):
        a.set_value_clip(mode, r)
        rows_a, _ = a.update(LR, CR, epochs, nmb, perms)                 # replayed
        b = make_update_handle(hidden, E, T, ro, orc.theta, state)
        b.set_value_clip(mode, r)
        rows_b, _ = b.update(LR, CR, epochs, nmb, perms)
        np.testing.assert_array_equal(rows_a, rows_b, err_msg="mode %d" % mode)
        np.testing.assert_array_equal(a.get_flat(0), b.get_flat(0), err_msg="mode %d" % mode)
        assert b.kernel_counts().get(key, 0) > 0, b.kernel_counts()
        if mode != POLICY:
            c = make_update_handle(hidden, E, T, ro, orc.theta, state)
            rows_c, _ = c.update(LR, CR, epochs, nmb, perms)
            assert not np.array_equal(rows_c[:, 1], rows_b[:, 1])           # the setting changes the update at all
            c.close()
        b.close()
        state = (a.get_flat(0), a.get_flat(1), a.get_flat(2), a.beta_powers())
    assert a.kernel_counts().get(key, 0) > 0
    a.close()


@pytest.mark.gpu
def test_update_matches_spliced_reference():
    """ppo_update in RANGE mode against the spliced reference driven minibatch by minibatch as Oracle.update does (env-major rows, explicit perms,
    per-minibatch advantage normalisation)"""
    hidden, E, T, nmb, epochs = (64, 64), 8, 32, 2, 2
    B, M = E * T, E * T // nmb
    orc = new_oracle(hidden)
    ro = rollout_inputs(orc, E, T)
    rng = np.random.RandomState(8)
    perms = np.stack([rng.permutation(B).astype(np.int32) for _ in range(epochs)])
    g = make_update_handle(hidden, E, T, ro, orc.theta)
    g.set_value_clip("range", R_VF)
    rows, mean = g.update(LR, CR, epochs, nmb, perms)
    assert g.kernel_counts().get("narrow_train_kernel<static>", 0) > 0
    ref_rows = mirrored_update(orc, ro, perms, nmb, LR, CR, RANGE, R_VF)
    close(rows[:, :4], ref_rows[:, :4], rtol=2e-4, atol=2e-6, msg="loss rows")
    assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= 1.01 / M)
    close(g.get_flat(0), orc.theta, rtol=2e-4, atol=5e-6, msg="theta")
    g.close()


def _explicit_inputs(E, T, U=1, epochs=2, A=18):
    orc = new_oracle((64, 64))
    rng = np.random.RandomState(77)
    noise = rng.normal(size=(U, T, E, A)).astype(np.float32)
    perms = np.empty((U, epochs, E * T), np.int32)
    for u in range(U):
        for e in range(epochs):
            perms[u, e] = rng.permutation(E * T)
    return orc.theta.copy(), noise, perms


@pytest.mark.gpu
@pytest.mark.parametrize("reference_loop", [False, True])
def test_host_learn_explicit_honours_cliprange_vf(reference_loop):
    from ppo_cpp_amd import hostapi
    E, T, nmb = 4, 32, 2
    theta, noise, perms = _explicit_inputs(E, T)
    run = lambda vf: hostapi.learn_explicit(E, T, [64, 64], theta, noise, perms, nmb, cliprange=CR, reference_loop=reference_loop, cliprange_vf=vf)
    default = run(-1.0)
    same = run(CR)
    other = run(R_VF)
    np.testing.assert_array_equal(same["theta"], default["theta"])
    np.testing.assert_array_equal(same["losses"], default["losses"])
    assert not np.array_equal(other["theta"], default["theta"])
    assert other["losses"][0][1] != default["losses"][0][1]


@pytest.mark.gpu
def test_checkpoint_restores_the_value_clip(tmp_path):
    from ppo_cpp_amd import hostapi
    assert hostapi.value_clip_checkpoint(str(tmp_path / "r"), 0.125) == (RANGE, pytest.approx(0.125))
    assert hostapi.value_clip_checkpoint(str(tmp_path / "off"), float("inf")) == (OFF, 0.0)
    assert hostapi.value_clip_checkpoint(str(tmp_path / "pol"), -1.0) == (POLICY, 0.0)


@pytest.mark.gpu
def test_driver_flag_runs_a_seeded_update(tmp_path):
    exe = os.path.join(ROOT, "ppo_cpp_amd", "ppo_cpp_hip")
    common = ["--seeded", "--threads", "2", "--batch_steps", "32", "--minibatches", "2", "--epochs", "2", "--steps", "64", "--seed", "3"]
    dumps = {}
    for tag, extra in (("default", []), ("off", ["--cliprange_vf", "off"]), ("cr", ["--cr_vf", "0.2"])):
        d = tmp_path / tag
        d.mkdir()
        out = subprocess.run([exe] + common + extra + ["--dump_dir", str(d)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        dumps[tag] = np.fromfile(str(d / "rank0.theta.f32"), np.float32)
    np.testing.assert_array_equal(dumps["cr"], dumps["default"])             # --cr defaults to 0.2: the same loss
    assert not np.array_equal(dumps["off"], dumps["default"])
