"""The multi-categorical head (and action masks) in the narrow LDS-resident kernels: ppo_create_multi_ex(cfg, nvec, K, PPO_ACT_SHAPE_KERNELS) /
PPOHip(action_dist="multi_categorical", nvec=.., shape_kernels=True) against tests/multi_categorical_ref.py.

A narrow workgroup is 32 rows (two pipes of 16) and a lane owns the columns part + 16 k, so the shapes are: the two static instantiations (odd offsets, a
component that straddles column 16; the learning run's head; K = 16, every lane holding a component), and the runtime shape with Ap = 64 and components of two
and three columns per lane, with the largest LDS image (64-column observation tile, 48 logit columns) and with tiny widths.  Row counts 1, 33 (a second workgroup
with one live row) and 200 (no multiple of 32).
Tolerances are the project's own (as written in tests/test_multi_discrete.py and tests/test_narrow_categorical.py).
(36, (2, 2, 2, 2, 20, 3, 33), (64, 64)) is a 64-column observation tile in front of 64 logit columns: the plain image would be about 173 KB, so this handle takes the
compact layout of build_narrow_layout (logits over dy[0], mask rows over dy[L-1]).  (50, (2, 17, 16, 5), (64, 64)) is the largest plain image, 158,096 bytes."""
import ctypes
import os

import numpy as np
import pytest

from tests import counter_draws_ref as draws_ref
from tests import truncation_ref as tr
from tests.masked_categorical_ref import random_masks as cat_random_masks
from tests.multi_categorical_ref import MultiCatRef, offsets, random_masks
from tests.test_multi_discrete import (CR, GAMMA, LAM, LR, TIE, check_actions, check_rollout, check_train_step, close, create_multi, make, ref_rollout,
                                       synth_batch, upload_and_update)
from tests.test_narrow_categorical import assert_padding_is_zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(18, (3, 5, 2, 8), (64, 64)),                    # static <32,64,32,2>: odd offsets; component 3 straddles column 16
          (36, (6, 6, 6), (64, 64)),                       # static <64,64,32,2>: the learning run's head
          (18, (2,) * 16, (64, 64)),                       # static; K = 16: every lane holds a component, the action row is as wide as it can be
          (36, (2, 2, 2, 2, 20, 3, 33), (64, 64)),         # runtime; Ap = 64, components with two and three columns per lane, K = 7
          (50, (2, 17, 16, 5), (64, 64)),                  # runtime; 64-column observation tile and 48 logit columns: the largest LDS image
          (7, (2, 3), (4, 5))]                             # runtime; tiny widths
ROWS = [1, 33, 200]
NEW = ("narrow_step_kernel<mcat>", "narrow_step_kernel<mcat,mask>", "narrow_train_kernel<mcat>", "narrow_train_kernel<mcat,mask>")
SHAPE_KERNELS = 0x100
LOGIT_TOL = 1e-4        # test 10: two fp32 evaluations of the same logits agree to 1e-4 (the value / neglogp tolerance)
DRAW = dict(O=18, nvec=(3, 5, 2, 8), hidden=(64, 64), n=200, weights=31, obs=4, seed=5)


def narrow(O, nvec, hidden, **kw):
    """(reference, handle created with the flag)"""
    return make(O, nvec, hidden, shape_kernels=True, **kw)


def assert_only_narrow_mcat(kc, **want):
    """the new names as asked for (name=count, or name=True for "at least once"); every other step / train name of every family, every Gaussian-only narrow form and
    the generic weight-gradient / reduce kernels: zero"""
    for name in NEW:
        assert name in kc, kc
    for name, cnt in want.items():
        name = dict(zip(("step", "step_mask", "train", "train_mask"), NEW))[name]
        assert (kc[name] > 0) if cnt is True else (kc[name] == cnt), (name, cnt, kc)
    for name, cnt in kc.items():
        if name not in NEW and name.startswith(("narrow_", "train8", "weight_grad", "grad_reduce", "bf16_", "policy_step_kernel", "train_fwd_bwd_kernel")):
            assert cnt == 0, (name, kc)


def step_inputs(O, nvec, n, masked):
    """the inputs of tests 5 and 6 (and of their input condition, test 4): (weight seed, observations, uniforms, masks or None)"""
    rng = np.random.RandomState(7 + 13 * n + O)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, sum(nvec))).astype(np.float32)
    mask = random_masks(rng, n, nvec) if masked else None          # the first rows: only the first category of every component, only the last, all
    return n, obs, u, mask


def counter_uniforms(seed, n, A, step=0):
    return draws_ref.counter_uniforms(draws_ref.seed_key(seed), np.arange(n), step, A).astype(np.float32)


def clear_pairs(ref, logits, u, tol):
    """[n, K] bool: the (row, component) pairs whose two best perturbed logits keep their order under a logit perturbation of tol (each may move by tol)"""
    pert = logits - np.log(-np.log(u.astype(np.float64)))
    return ref.top2_gap(pert) > 2 * tol


def draw_inputs():
    d = DRAW
    obs = np.random.RandomState(d["obs"]).uniform(-1, 1, (d["n"], d["O"])).astype(np.float32)
    return obs, counter_uniforms(d["seed"], d["n"], sum(d["nvec"]))


def create_multi_ex(nvec, flags, act_dim=None, n_components=None, **overrides):
    """ppo_create_multi_ex through ctypes; returns (status, message)"""
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, sum(nvec) if act_dim is None else act_dim, 2, hid)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    nv = (ctypes.c_int32 * 32)(*nvec)
    rc = lib.ppo_create_multi_ex(ctypes.byref(cfg), nv, len(nvec) if n_components is None else n_components, flags, ctypes.byref(h))
    msg = lib.ppo_last_error(None).decode() if rc != 0 else ""
    if rc == 0:
        lib.ppo_destroy(h)
    return rc, msg


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_create_multi_ex(const ppo_config* cfg, const int32_t* nvec, int32_t n_components, int32_t flags, ppo_handle** out);" in src
    assert "int ppo_create_multi(const ppo_config* cfg, const int32_t* nvec, int32_t n_components, ppo_handle** out);" in src
    assert "#define PPO_ABI_VERSION 3" in src and "#define PPO_ACT_SHAPE_KERNELS 0x100" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    assert hasattr(lib, "ppo_create_multi_ex") and hasattr(lib, "ppo_create_multi")
    assert lib.ppo_abi_version() == 3
    for name in NEW:
        assert len(name) < 32           # ppo_kernel_counts' char[32]


def test_creation_errors_of_the_flagged_entry_point():
    """(checked before a device is looked for: the same messages with and without a GPU)"""
    rc, msg = create_multi_ex([3, 5], 0x800)
    assert rc != 0 and "ppo_create_multi_ex" in msg and "0x800" in msg, msg
    rc, msg = create_multi_ex([3, 5], SHAPE_KERNELS | 0x1)
    assert rc != 0 and "ppo_create_multi_ex" in msg and "0x1" in msg, msg
    cases = [dict(nvec=[], act_dim=4, n_components=0), dict(nvec=[2] * 17), dict(nvec=[3, 1, 4]), dict(nvec=[3, 5], act_dim=9), dict(nvec=[3, 5], compute_dtype=1)]
    for kw in cases:
        nvec = kw.pop("nvec")
        rc0, msg0 = create_multi(nvec, **kw)
        assert rc0 != 0 and msg0.startswith("ppo_create_multi: "), msg0
        for flags in (0, SHAPE_KERNELS, SHAPE_KERNELS | 0x200 | 0x400):
            rc, msg = create_multi_ex(nvec, flags, **kw)
            assert rc != 0 and msg == msg0, (flags, msg, msg0)
    for flags in (0, SHAPE_KERNELS, 0x200, 0x400):                  # PPO_BF16 stays refused, whatever the flags
        rc, msg = create_multi_ex([3, 5], flags, compute_dtype=1)
        assert rc != 0 and "PPO_BF16" in msg, msg


def test_python_layers_accept_the_flag():
    import inspect
    import ppo_cpp_amd
    from ppo_cpp_amd import hostapi
    assert inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters["shape_kernels"].default is False
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="no CPU fallback"):
            ppo_cpp_amd.PPOHip(18, None, [64, 64], action_dist="multi_categorical", nvec=[3, 5], shape_kernels=True)
    assert hostapi._discrete_kernels("generic") == 0 and hostapi._discrete_kernels("narrow") == 1 and hostapi._discrete_kernels("pair") == 2
    with pytest.raises(ValueError, match="discrete_kernels"):
        hostapi._discrete_kernels("wide")


@pytest.mark.parametrize("O,nvec,hidden", SHAPES)
def test_reference_alone_has_no_more_near_ties_than_the_action_checks_allow(O, nvec, hidden):
    """the input condition of tests 5 and 6: under the float64 reference ALONE, with those tests' own seeds, the near-tie count of check_actions is within its cap
    pairs // 1000 (zero for the small cases) for the sampled and the deterministic actions, unmasked and masked"""
    for n in ROWS:
        for masked in (False, True):
            seed, obs, u, mask = step_inputs(O, nvec, n, masked)
            ref = MultiCatRef(O, nvec, hidden)
            ref.init_random(seed)
            _, _, _, pert = ref.step(obs, u, mask)
            logits = ref.forward(obs)[0]
            plain = logits if mask is None else np.where(mask != 0, logits, -np.inf)
            for what, x in (("sampled", pert), ("deterministic", plain)):
                ties = int((ref.top2_gap(x) < TIE).sum())
                assert ties <= (n * len(nvec)) // 1000, (what, n, masked, ties)


def test_reference_alone_has_clear_margins_for_the_draw_comparison():
    """test 10's input condition (the rule of tests/test_narrow_categorical.py's test of this name, per (row, component) pair): under the reference alone, with the
    kernels' own counter uniforms, at least 0.9 of the pairs keep their category under a logit perturbation of LOGIT_TOL"""
    d = DRAW
    ref = MultiCatRef(d["O"], d["nvec"], d["hidden"])
    ref.init_random(d["weights"])
    obs, u = draw_inputs()
    assert u.min() > 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02
    share = float(clear_pairs(ref, ref.forward(obs)[0], u, LOGIT_TOL).mean())
    print("clear-margin pairs under the reference: %.4f" % share)
    assert share >= 0.9


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def check_step(O, nvec, hidden, n, masked):
    seed, obs, u, mask = step_inputs(O, nvec, n, masked)
    ref, g = narrow(O, nvec, hidden, seed=seed)
    K = len(nvec)
    assert g.lib.ppo_action_dist(g.h) == 2 and g.nvec == list(nvec) and g.action_width == K
    a, v, nlp = g.step(obs, u, mask=mask)
    assert a.shape == (n, K) and v.shape == (n,) and nlp.shape == (n,)
    ra, rv, _, pert = ref.step(obs, u, mask)
    check_actions(ref, a, ra, pert, "sampled actions")
    logits = ref.forward(obs)[0]
    close(nlp, ref.neglogp_of(logits, a, mask), atol=1e-5 * K, msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    det = g.act_deterministic(obs, mask=mask)
    assert det.shape == (n, K)
    check_actions(ref, det, ref.act_deterministic(obs, mask), logits if mask is None else np.where(mask != 0, logits, -np.inf), "deterministic actions")
    g.seed(3)
    a2, _, nlp2 = g.step(obs, mask=mask)
    assert np.all(a2 == np.floor(a2)) and a2.min() >= 0 and np.all(a2 < np.array(nvec))
    close(nlp2, ref.neglogp_of(logits, a2, mask), atol=1e-5 * K, msg="neglogp of the counter draw")
    if masked:
        cols = offsets(nvec)[:-1]
        for acts in (a, det, a2):                                 # no forbidden category, near-tie or not
            assert np.all(np.take_along_axis(mask, acts.astype(np.int64) + cols, 1) != 0)
        single = np.all(np.stack([ref.comp(mask, k).sum(1) == 1 for k in range(K)], 1), 1)   # rows whose every component allows ONE category
        assert single[0] and np.all(np.abs(nlp[single]) <= 1e-6) and np.all(np.abs(nlp2[single]) <= 1e-6), (nlp[single], nlp2[single])
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,hidden", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_step_matches_reference(O, nvec, hidden, n):
    g = check_step(O, nvec, hidden, n, False)
    assert_only_narrow_mcat(g.kernel_counts(), step=4, step_mask=0)      # step, ppo_value, deterministic act, the counter draw
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,hidden", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_masked_step_matches_reference(O, nvec, hidden, n):
    g = check_step(O, nvec, hidden, n, True)
    assert_only_narrow_mcat(g.kernel_counts(), step_mask=3, step=1)      # (ppo_value takes no mask)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,nvec,hidden", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_three_train_steps_match_reference(O, nvec, hidden, masked):
    """the tolerances of tests/test_narrow_categorical.py's test of this name"""
    n = 200
    ref, g = narrow(O, nvec, hidden, seed=9, ent_coef=0.01)
    dead = int(offsets(nvec)[1])                           # masked: the first category of component 1 is forbidden in EVERY row (its neighbour always allowed)
    o_w, s_w = ref.offs["pi/w"]
    o_b, _ = ref.offs["pi/b"]
    assert_padding_is_zero(g)
    g.prof_enable(True)
    gmax = 0.0
    for it in range(3):
        mask = None
        if masked:
            mask = random_masks(np.random.RandomState(50 + it), n, nvec)
            mask[:, dead] = 0.0
            mask[:, dead + 1] = 1.0
        batch = synth_batch(ref, n, 100 + it, mask=mask)
        losses = g.train_step(LR, CR, *batch, mask=mask)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch, mask=mask)
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        gmax = max(gmax, gs)
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
        if masked:
            gw = grad[o_w:o_w + s_w[0] * s_w[1]].reshape(s_w)
            assert np.all(gw[:, dead] == 0.0) and grad[o_b + dead] == 0.0, "the forbidden category's column / bias entry must get an exactly zero gradient"
            assert np.any(gw[:, :dead] != 0.0)            # (component 0's columns; the neighbour's own gradient is 0 where it is its component's only allowed category)
    close(g.get_flat(2), ref.v, rtol=4e-4, atol=1.2e-5 * (1.0 - ref.b2) * gmax * gmax, msg="adam v after the third step")
    assert_padding_is_zero(g)                              # the padded logstd slot among it: Adam never moved it
    kc = g.kernel_counts()
    assert_only_narrow_mcat(kc, **({"train_mask": 3, "train": 0} if masked else {"train": 3, "train_mask": 0}))
    prof = g.prof_read()                                   # narrow_reduce_kernel: the timed "grad_reduce" class ran once per step while grad_reduce_kernel never did
    assert prof["grad_reduce"][1] == 3 and kc["grad_reduce_kernel"] == 0 and prof.get("weight_grad", (0, 0))[1] == 0, (prof, kc)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A", [(18, 6), (50, 40)])       # the static instantiation; the runtime one with the largest image
def test_one_component_is_the_categorical_narrow_handle_bit_for_bit(O, A):
    import ppo_cpp_amd
    n, hidden = 200, (64, 64)
    ref, gm = narrow(O, [A], hidden, seed=2, ent_coef=0.01)
    gc = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", shape_kernels=True, ent_coef=0.01)
    gc.set_flat(ref.theta.astype(np.float32))
    rng = np.random.RandomState(3)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    rmask = cat_random_masks(rng, n, A)

    def same_step(noise, mask):
        (am, vm, nm), (ac, vc, nc) = gm.step(obs, noise, mask=mask), gc.step(obs, noise, mask=mask)
        assert am.shape == (n, 1) and ac.shape == (n,)
        np.testing.assert_array_equal(am[:, 0], ac); np.testing.assert_array_equal(vm, vc); np.testing.assert_array_equal(nm, nc)
        np.testing.assert_array_equal(gm.act_deterministic(obs, mask=mask)[:, 0], gc.act_deterministic(obs, mask=mask))

    for mask in (None, rmask):
        same_step(u, mask)
        gm.seed(11); gc.seed(11)
        same_step(None, mask)
        for it in range(2):
            obs_b, a, adv, ret, nlp, v = synth_batch(ref, n, 30 + it, mask=mask)
            lm = gm.train_step(LR, CR, obs_b, a, adv, ret, nlp, v, mask=mask)
            lc = gc.train_step(LR, CR, obs_b, a[:, 0], adv, ret, nlp, v, mask=mask)
            np.testing.assert_array_equal(lm, lc)
            (g1, n1), (g2, n2) = gm.last_grad(), gc.last_grad()
            np.testing.assert_array_equal(g1, g2)
            assert n1 == n2
            for which in (0, 1, 2):
                np.testing.assert_array_equal(gm.get_flat(which), gc.get_flat(which))
    assert_only_narrow_mcat(gm.kernel_counts(), step=True, step_mask=True, train=2, train_mask=2)
    kc = gc.kernel_counts()
    assert kc["narrow_train_kernel<cat>"] == 2 and kc["narrow_train_kernel<cat,mask>"] == 2 and all(kc[name] == 0 for name in NEW), kc
    gm.close(); gc.close()


@pytest.mark.gpu
def test_all_ones_masks_give_the_unmasked_bits():
    O, nvec, hidden, n, E, T = 18, (3, 5, 2, 8), (64, 64), 100, 32, 8
    ref, g1 = narrow(O, nvec, hidden, seed=6, ent_coef=0.01)
    _, g2 = narrow(O, nvec, hidden, seed=6, ent_coef=0.01)
    rng = np.random.RandomState(9)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, ref.A)).astype(np.float32)
    ones = np.ones((n, ref.A), np.float32)
    for x, y in zip(g1.step(obs, u), g2.step(obs, u, mask=ones)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(g1.act_deterministic(obs), g2.act_deterministic(obs, mask=ones))
    batch = synth_batch(ref, n, 60)
    np.testing.assert_array_equal(g1.train_step(LR, CR, *batch), g2.train_step(LR, CR, *batch, mask=ones))
    np.testing.assert_array_equal(g1.last_grad()[0], g2.last_grad()[0])
    for which in (0, 1, 2):
        np.testing.assert_array_equal(g1.get_flat(which), g2.get_flat(which))
    g2.set_action_masking(True)                                # masks default to ones
    ro = ref_rollout(ref, 77, E, T, rng.uniform(size=(T, E, ref.A)).astype(np.float32))
    perms = np.stack([rng.permutation(E * T) for _ in range(2)]).astype(np.int32)
    outs = []
    for g in (g1, g2):
        g.norm_init(E)
        g.rollout_alloc(E, T)
        for f in ("obs", "actions", "values", "neglogp", "returns"):
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        rows, mean = g.update(LR, CR, 2, 4, perms)
        outs.append((rows, mean, g.get_flat(0), g.get_flat(1), g.get_flat(2)))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    assert_only_narrow_mcat(g1.kernel_counts(), step=True, train=True, step_mask=0, train_mask=0)
    assert_only_narrow_mcat(g2.kernel_counts(), step_mask=True, train_mask=True, train=0)
    g1.close(); g2.close()


@pytest.mark.gpu
def test_same_seed_same_draw_as_the_generic_family():
    d = DRAW
    K = len(d["nvec"])
    ref, gn = narrow(d["O"], d["nvec"], d["hidden"], seed=d["weights"])
    _, gg = make(d["O"], d["nvec"], d["hidden"], seed=d["weights"])
    obs, u = draw_inputs()
    out = []
    for g in (gg, gn):
        g.seed(d["seed"])
        out.append(g.step(obs))
    (ag, vg, nlpg), (an, vn, nlpn) = out
    assert gg.kernel_counts()["policy_step_kernel<mcat>"] == 1 and gn.kernel_counts()["narrow_step_kernel<mcat>"] == 1
    assert all(gg.kernel_counts()[name] == 0 for name in NEW)              # an unflagged handle never counts the new names
    logits = ref.forward(obs)[0]
    clear = clear_pairs(ref, logits, u, LOGIT_TOL)
    ra = ref.step(obs, u)[0].astype(np.float32)
    print("pairs compared: %.4f" % clear.mean())
    assert clear.mean() >= 0.9
    np.testing.assert_array_equal(ag[clear], ra[clear])
    np.testing.assert_array_equal(an[clear], ra[clear])
    np.testing.assert_array_equal(an[clear], ag[clear])
    close(vn, vg, msg="values")
    same = np.all(an == ag, axis=1)
    close(nlpn[same], nlpg[same], atol=1e-5 * K, msg="neglogp")
    gg.close(); gn.close()


def device_env_case(E, T=4, O=18, nvec=(3, 5, 2, 8)):
    """collect_synthetic against the reference, then two updates with explicit permutations; returns what the run left behind"""
    ref, g = narrow(O, nvec, (64, 64), seed=E, ent_coef=0.01)
    u = np.random.RandomState(E).uniform(size=(T, E, ref.A)).astype(np.float32)
    ro = ref_rollout(ref, 1234, E, T, u)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(1234, GAMMA, LAM, u)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns")}
    assert got["actions"].shape == (T, E, len(nvec))
    check_rollout(ref, got, ro, "collect E=%d" % E)
    rng = np.random.RandomState(3)
    for it in range(2):
        ro = ref_rollout(ref, 500 + it, E, T, rng.uniform(size=(T, E, ref.A)).astype(np.float32))
        ro["obs"] = ro["obs"].astype(np.float32)
        upload_and_update(ref, g, ro, rng, E, T, 4, 2, it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    kc = g.kernel_counts()
    left = dict(theta=g.get_flat(0), m=g.get_flat(1), v=g.get_flat(2), rms=g.norm_stats(0), ret_rms=g.norm_stats(1), **got)
    g.close()
    return kc, left


@pytest.mark.gpu
@pytest.mark.parametrize("E", [3, 40])                     # 40: a second workgroup with 8 live rows
def test_collect_synthetic_and_updates_match_reference(E):
    kc, a = device_env_case(E)
    # (an update is captured into a hipGraph once and replayed: the counts are those of the capture, epochs x minibatches)
    assert_only_narrow_mcat(kc, step=True, train=True, step_mask=0, train_mask=0)
    if E == 40:                                            # the same case again: the same bits in every field, statistic and flat vector
        _, b = device_env_case(E)
        for k in a:
            if k in ("rms", "ret_rms"):
                for x, y in zip(a[k], b[k]):
                    np.testing.assert_array_equal(x, y)
            else:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.gpu
def test_host_env_loop_with_masks_and_updates_match_reference():
    from oracle import oracle as o
    O, nvec, E, T = 18, (3, 5, 2, 8), 40, 4
    ref, g = narrow(O, nvec, (64, 64), seed=41, ent_coef=0.01)
    g.set_action_masking(True)
    rng = np.random.RandomState(E + 1)
    u = rng.uniform(size=(T, E, ref.A)).astype(np.float32)
    masks = np.stack([random_masks(rng, E, nvec) for _ in range(T)])
    ro = ref_rollout(ref, 99, E, T, u, masks)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, u[t], mask=masks[t])
        assert a.shape == (E, len(nvec))
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in ("obs", "actions", "values", "neglogp", "rewards", "returns")}
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    np.testing.assert_array_equal(g.rollout_get("masks"), masks)
    check_rollout(ref, got, ro, "host Env")
    rng = np.random.RandomState(3)
    for it in range(2):
        mk = np.stack([random_masks(rng, E, nvec) for _ in range(T)])
        ro = ref_rollout(ref, 500 + it, E, T, rng.uniform(size=(T, E, ref.A)).astype(np.float32), mk)
        ro["obs"] = ro["obs"].astype(np.float32)
        upload_and_update(ref, g, ro, rng, E, T, 4, 2, it)
    kc = g.kernel_counts()
    assert kc["grad_reduce_kernel"] == 0, kc
    assert_only_narrow_mcat(kc, step_mask=T, train_mask=True, step=1, train=0)      # (step: the bootstrap value of rollout_finish)
    g.close()


@pytest.mark.gpu
def test_truncation_bootstrap_uses_the_narrow_value_pass():
    O, nvec, E, T = 18, (3, 5, 2, 8), 3, 6
    ref, g = narrow(O, nvec, (64, 64), seed=9)
    rng = np.random.RandomState(12)
    step_dones = np.zeros((T, E), np.float32)
    trunc = np.zeros((T, E), bool)
    step_dones[2, 1] = 1.0; trunc[2, 1] = True                    # one marked row
    step_dones[4, 0] = 1.0                                        # and a real terminal state
    term_raw = rng.uniform(-1.5, 1.5, (T, E, O)).astype(np.float32)
    noise = rng.uniform(size=(T, E, ref.A)).astype(np.float32)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    tr.host_rollout(g, 321, E, T, step_dones, trunc, term_raw, GAMMA, LAM, noise)
    want = tr.ref_rollout(g, 321, E, T, step_dones, trunc, term_raw, GAMMA, LAM)
    tv = g.rollout_get("terminal_values")
    close(g.rollout_get("values"), want["values"], rtol=2e-4, atol=2e-5, msg="values")
    close(tv[trunc], want["terminal_values"][trunc], rtol=2e-4, atol=2e-5, msg="terminal values")
    assert np.all(tv[~trunc] == 0.0) and abs(want["terminal_values"][2, 1]) > 1e-3
    close(g.rollout_get("returns"), want["returns"], rtol=2e-4, atol=2e-5, msg="returns")
    kc = g.kernel_counts()
    assert kc["tval_scatter_kernel"] == 1, kc
    assert_only_narrow_mcat(kc, step=T + 2, step_mask=0)          # T act steps, the bootstrap, the value-only pass
    g.close()


def assert_generic_mcat(kc, step, train):
    assert kc["policy_step_kernel<mcat>"] == step and kc["train_fwd_bwd_kernel<mcat>"] == train and not any(c for k, c in kc.items() if k.startswith("narrow_")), kc


@pytest.mark.gpu
def test_fallbacks_and_errors(monkeypatch):
    import ppo_cpp_amd
    rng = np.random.RandomState(1)
    n = 33
    # shapes that do not qualify: the generic <mcat> kernels, silently, with the reference's results
    for O, nvec, hidden in [(18, (3, 5, 2, 8), (256, 256)), (18, (2, 17, 16, 17, 13), (64, 64))]:        # hidden width; 65 logits
        ref, g = narrow(O, nvec, hidden, seed=2)
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
        u = rng.uniform(size=(n, ref.A)).astype(np.float32)
        a, v, nlp = g.step(obs, u)
        ra, rv, _, pert = ref.step(obs, u)
        check_actions(ref, a, ra, pert, "fallback actions")
        close(v, rv, msg="value"); close(nlp, ref.neglogp_of(ref.forward(obs)[0], a), atol=1e-5 * ref.K, msg="neglogp")
        check_train_step(ref, g, synth_batch(ref, 64, 1), None, 64, 0)
        assert_generic_mcat(g.kernel_counts(), 1, 1)
        g.close()
    O, nvec, hidden = 18, (3, 5, 2, 8), (64, 64)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    # an unflagged handle: zero for the four new names, and data parallel stays available to it
    ref, g = make(O, nvec, hidden)
    g.step(obs)
    assert_generic_mcat(g.kernel_counts(), 1, 0)
    assert all(g.kernel_counts()[name] == 0 for name in NEW)
    g.close()
    # data parallel on a handle the flag took effect on: refused with its message; the handle stays usable
    ref, g = narrow(O, nvec, hidden)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="data parallel is not supported for a multi-categorical handle created with PPO_ACT_SHAPE_KERNELS"):
        g.dist_init(1, 0, bytes(128))
    g.step(obs)
    assert g.kernel_counts()["narrow_step_kernel<mcat>"] == 1
    # the host checks are the generic handle's
    batch_obs, a, adv, ret, nlp, v = synth_batch(ref, 32, 0)
    theta = g.get_flat(0)
    for bad in (5.0, -1.0, 2.5, np.nan):                       # component 1 has 5 categories
        a2 = a.copy(); a2[5, 1] = bad
        with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 5, component 1.*\[0, 5\)"):
            g.train_step(LR, CR, batch_obs, a2, adv, ret, nlp, v)
    ones = np.ones((32, ref.A), np.float32)
    m2 = ones.copy(); m2[7, 3:8] = 0.0                          # component 1 of row 7 fully forbidden
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.step(batch_obs, mask=m2)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.train_step(LR, CR, batch_obs, a, adv, ret, nlp, v, mask=m2)
    m3 = ones.copy(); m3[9, 10 + int(a[9, 3])] = 0.0            # row 9's own action in component 3 (offset 10)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 9, component 3.*forbidden"):
        g.train_step(LR, CR, batch_obs, a, adv, ret, nlp, v, mask=m3)
    np.testing.assert_array_equal(g.get_flat(0), theta)          # nothing was trained
    g.close()
    # PPO_HIP_NO_NARROW=1 with the flag: the generic kernels
    monkeypatch.setenv("PPO_HIP_NO_NARROW", "1")
    _, g = narrow(O, nvec, hidden)
    g.step(obs)
    assert_generic_mcat(g.kernel_counts(), 1, 0)
    g.close()


@pytest.mark.gpu
def test_ppo2_learns_the_multi_discrete_target_task_on_the_narrow_kernels():
    """tests/test_multi_discrete.test_ppo2_learns_the_multi_discrete_target_task with discrete_kernels="narrow": the same task, the same RISE / BAND / reference figure
    (they come from the NumPy reference loop; see there)."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.123, 0.089, 0.419
    got = hostapi.learn_curve(16, 64, [64, 64], 80, 4, 4, 2e-3, 0.2, seed=11, nvec=(6, 6, 6), discrete_kernels="narrow")
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    assert_only_narrow_mcat(got["kernel_counts"], step=True, train=True, step_mask=0, train_mask=0)
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)


@pytest.mark.gpu
@pytest.mark.parametrize("reference_loop", [False, True])
def test_ppo2_runs_the_masked_multi_discrete_env_on_the_narrow_kernels(reference_loop):
    from ppo_cpp_amd import hostapi
    got = hostapi.learn_curve(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, nvec=(6, 6, 6), masked=True, n_playback=30, reference_loop=reference_loop,
                              discrete_kernels="narrow")
    assert got["forbidden_received"] == 0
    assert got["playback_actions"].shape == (30, 3) and np.all(got["playback_legal"] == 1.0)
    assert np.all(got["reward_curve"] >= 0.0)
    assert_only_narrow_mcat(got["kernel_counts"], step_mask=True, train_mask=True, train=0)
