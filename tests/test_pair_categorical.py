"""The categorical head (and action masks) in the [256,256] kernel pair: PPO_ACT_CATEGORICAL | PPO_ACT_PAIR_KERNELS (include/ppo_hip.h) /
PPOHip(action_dist="categorical", pair_kernels=True) runs train8_kernel<cat[,mask]> + weight_grad_assemble_kernel instead of the generic four launches.

References: the float64 CatRef / MaskedCatRef of tests/categorical_ref.py and tests/masked_categorical_ref.py.  Tolerances: those of
tests/test_discrete_policy.py and tests/test_action_mask.py for the same quantity (losses, clipfrac within one row, gradient, norm, weights, Adam m);
where a case has more than 32 categories the gradient takes the pair's own Gaussian bound (tests/test_other_shapes.py, atol 4e-6 of the largest element:
the head gradient then has thousands of elements three orders below the largest).  The Adam v slot, which those files do not check, follows from the
gradient's bound: v is a (1 - beta2)-weighted sum of g^2 over the steps, so rtol is twice the gradient's and atol = steps * (1 - beta2) * 2 gs * atol_g.
Hidden [256,256] is fixed by the kernel; every other size is the smallest that reaches the code (16 and 100 rows: one live tile with three dead ones
behind it, and a last live tile with dead rows inside plus a dead tile)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests.masked_categorical_ref import MaskedCatRef, random_masks
from tests.test_action_mask import synth_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CR = 0.16102319955825806
LR = 0.000393141177482903
HID = (256, 256)
# one (O, A) per instantiation <KP0, AP>: <32,32>, <64,32>, <32,64>, <64,64> (a full 64-column tile), and A = 33: the second element of only one lane is live
SHAPES = [(18, 6), (36, 18), (18, 40), (50, 64), (18, 33)]


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_flag_and_keeps_the_abi():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_PAIR_KERNELS 0x400" in src
    assert "#define PPO_ABI_VERSION 3" in src
    assert '"train8_kernel<cat>", "train8_kernel<cat,mask>"' in src
    assert "data parallel is not supported for a categorical handle created with PPO_ACT_PAIR_KERNELS" in src


def test_pair_kernels_is_an_opt_in_keyword():
    import ppo_cpp_amd
    from ppo_cpp_amd import capi
    assert capi.ACT_PAIR_KERNELS == 0x400
    p = inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters
    assert "pair_kernels" in p and p["pair_kernels"].default is False


def test_hostapi_accepts_pair():
    from ppo_cpp_amd import hostapi
    assert hostapi._discrete_kernels("generic") == 0 and hostapi._discrete_kernels("narrow") == 1 and hostapi._discrete_kernels("pair") == 2
    with pytest.raises(ValueError, match="discrete_kernels"):
        hostapi._discrete_kernels("wide")
    assert inspect.signature(hostapi.learn_curve).parameters["discrete_kernels"].default == "generic"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, A, hidden=HID, seed=0, pair=True, masking=False, ref=True, **overrides):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", pair_kernels=pair, **overrides)
    c = g.cfg
    r = MaskedCatRef(O, A, hidden, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, beta1=c.adam_beta1, beta2=c.adam_beta2, eps=c.adam_eps)
    r.init_random(seed)
    g.set_flat(r.theta.astype(np.float32))
    if masking:
        g.set_action_masking(True)
    return r, g


def delta(after, before):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def masks_for(n, A, seed):
    """random masks; the first rows are the special ones of random_masks (only category 0, only category A - 1: a row whose action is its only allowed category)"""
    return random_masks(np.random.RandomState(seed), n, A, special=True)


def check_step(g, ref, batch, mask, n, A, it, steps_so_far):
    """one train step of `g` against the same step of `ref`: losses, clipfrac within one row, gradient, clipped norm, weights, both Adam slots"""
    kw = {} if mask is None else {"mask": mask}
    losses = g.train_step(LR, CR, *batch, **kw)
    grad, norm = g.last_grad()
    ref_losses, ref_grad = ref.train_step(LR, CR, *batch, **kw)
    print("it %d losses %s ref %s" % (it, losses, ref_losses))
    close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
    assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
    gs = np.abs(ref_grad).max()
    atol_g = (4e-6 if A > 32 else 2e-6) * gs
    print("   grad max abs err %.3g (atol %.3g, largest %.3g)" % (np.abs(grad - ref_grad).max(), atol_g, gs))
    close(grad, ref_grad, rtol=2e-4, atol=atol_g, msg="grad it=%d" % it)
    close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
    close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
    close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
    close(g.get_flat(2), ref.v, rtol=4e-4, atol=(steps_so_far + 1) * (1.0 - ref.b2) * 2.0 * gs * atol_g, msg="adam v it=%d" % it)
    return losses, grad


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", [100, 16])
@pytest.mark.parametrize("O,A", SHAPES)
def test_three_train_steps_match_reference(O, A, n, masked):
    ref, g = make(O, A, seed=9, ent_coef=0.01)
    k0 = g.kernel_counts()
    for it in range(3):
        mask = masks_for(n, A, 200 + it) if masked else None
        batch = synth_batch(ref, n, 100 + it, mask)
        if masked:
            assert (mask.sum(1) == 1).any() and np.all(mask[np.arange(n), batch[1].astype(np.int64)] != 0)
        check_step(g, ref, batch, mask, n, A, it, it)
    assert delta(g.kernel_counts(), k0) == {"train8_kernel<cat,mask>" if masked else "train8_kernel<cat>": 3, "weight_grad_assemble_kernel": 3}
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("O,A", [(18, 18), (18, 40)])
def test_mask_semantics(O, A):
    """a row of ones gives the unmasked bits in every output; a category forbidden in the whole minibatch gets exactly 0 in its pi/w column and pi/b entry"""
    n, dead = 100, 5
    ref, g0 = make(O, A, seed=4, ent_coef=0.01)
    _, g1 = make(O, A, seed=4, ent_coef=0.01)
    ones = np.ones((n, A), np.float32)
    for it in range(2):
        batch = synth_batch(ref, n, 11 + it)
        np.testing.assert_array_equal(g0.train_step(LR, CR, *batch), g1.train_step(LR, CR, *batch, mask=ones))
        for x, y in zip(g0.last_grad(), g1.last_grad()):
            np.testing.assert_array_equal(x, y)
        for which in range(3):
            np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    kc0, kc1 = g0.kernel_counts(), g1.kernel_counts()
    assert kc0["train8_kernel<cat>"] == 2 and kc0["train8_kernel<cat,mask>"] == 0, kc0
    assert kc1["train8_kernel<cat,mask>"] == 2 and kc1["train8_kernel<cat>"] == 0, kc1
    g0.close()
    ref.theta[:] = g1.get_flat(0)
    o_w, s_w = ref.offs["pi/w"]
    o_b, _ = ref.offs["pi/b"]
    mask = random_masks(np.random.RandomState(7), n, A, special=False)
    mask[:, dead] = 0.0
    mask[mask.sum(1) == 0, 0] = 1.0
    mask[3] = 0.0; mask[3, A - 1] = 1.0                       # a row whose action is its only allowed category (the last one: the second element's lane at A = 40)
    batch = synth_batch(ref, n, 13, mask)
    assert batch[1][3] == A - 1
    losses = g1.train_step(LR, CR, *batch, mask=mask)
    assert np.isfinite(losses).all()
    grad, _ = g1.last_grad()
    gw = grad[o_w:o_w + s_w[0] * s_w[1]].reshape(s_w)
    assert np.all(gw[:, dead] == 0.0) and grad[o_b + dead] == 0.0, "the forbidden category's column / bias entry must get an exactly zero gradient"
    assert np.any(gw[:, dead - 1] != 0.0) and grad[o_b + dead - 1] != 0.0
    _, ref_grad = ref.loss_grad(*batch, CR, mask)
    close(grad, ref_grad, rtol=2e-4, atol=(4e-6 if A > 32 else 2e-6) * np.abs(ref_grad).max(), msg="masked gradient")
    g1.close()


def padded_logstd_region(O, A):
    """(offset, width) of pi/logstd in the padded parameter vector, read off a Gaussian handle of the same shape: a categorical handle keeps the region without a tensor"""
    import ppo_cpp_amd
    gauss = ppo_cpp_amd.PPOHip(O, A, list(HID))
    flat = np.zeros(gauss.P, np.float32)
    assert gauss.tensors[-1][0] == "pi/logstd"
    flat[-A:] = 7.0                                              # pi/logstd is the last tensor of the flat vector
    gauss.set_flat(flat)
    theta = gauss.debug_buffer("theta").view(np.float32)
    at = np.nonzero(theta == 7.0)[0]
    size = theta.size
    gauss.close()
    assert at.size == A and np.all(np.diff(at) == 1)
    width = 32 if A <= 32 else 64
    return int(at[0]), width, size


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_flagged_against_unflagged(masked):
    O, A, n = 18, 40, 100
    ref, gp = make(O, A, seed=6, ent_coef=0.01)
    _, gg = make(O, A, seed=6, ent_coef=0.01, pair=False)
    off, width, size = padded_logstd_region(O, A)
    before = {k: gp.debug_buffer(k).view(np.float32).copy() for k in ("theta", "adam_m", "adam_v")}
    assert before["theta"].size == size
    # every padding element of the vector (the logstd region among them): where a flat vector of ones does not land
    _, probe = make(O, A, seed=6)
    probe.set_flat(np.ones(probe.P, np.float32))
    pad = probe.debug_buffer("theta").view(np.float32) != 1.0
    probe.close()
    assert pad[off:off + width].all() and pad.sum() == size - gp.P
    rng = np.random.RandomState(5)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = masks_for(n, A, 3) if masked else None
    kw = {"mask": mask} if masked else {}
    for x, y in zip(gp.step(obs, u, **kw), gg.step(obs, u, **kw)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(gp.act_deterministic(obs, **kw), gg.act_deterministic(obs, **kw))
    for it in range(3):
        batch = synth_batch(ref, n, 40 + it, mask)
        lp, lg = gp.train_step(LR, CR, *batch, **kw), gg.train_step(LR, CR, *batch, **kw)
        ref.train_step(LR, CR, *batch, **kw)
        close(lp[:4], lg[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(lp[4] - lg[4]) <= 1.0 / n + 1e-6
        (grp, np_), (grg, ng) = gp.last_grad(), gg.last_grad()
        close(grp, grg, rtol=2e-4, atol=4e-6 * np.abs(grg).max(), msg="grad it=%d" % it)
        close(np_, ng, rtol=1e-4, msg="norm")
        close(gp.get_flat(0), gg.get_flat(0), rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
    kp, kg = gp.kernel_counts(), gg.kernel_counts()
    name = "<cat,mask>" if masked else "<cat>"
    assert kp["train8_kernel" + name] == 3 and kp["train_fwd_bwd_kernel" + name] == 0 and kp["weight_grad_assemble_kernel"] == 3, kp
    assert kg["train_fwd_bwd_kernel" + name] == 3 and kg["train8_kernel" + name] == 0 and kg["weight_grad_assemble_kernel"] == 0, kg
    assert kp["policy_step_kernel" + name] == kg["policy_step_kernel" + name] > 0, (kp, kg)           # the act kernels are the same
    for k, b in before.items():
        now = gp.debug_buffer(k).view(np.float32)
        np.testing.assert_array_equal(now[off:off + width], b[off:off + width], err_msg="padded logstd region of " + k)
        np.testing.assert_array_equal(now[pad], b[pad], err_msg="padding of " + k)
        assert not b[pad].any()
    gtail = gp.debug_buffer("grad").view(np.float32)
    assert not gtail[off:off + width].any(), "the padded logstd region of the gradient holds zeros on the pair path"
    gp.close(); gg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_update_matches_reference_and_replays(masked):
    """16 environments x 16 steps, 4 minibatches (64 rows each), 2 epochs, explicit permutations; the second update replays the captured graph"""
    from tests.test_action_mask import ref_rollout
    O, A, E, T, nmb, epochs = 18, 18, 16, 16, 4, 2
    ref, g = make(O, A, seed=17, ent_coef=0.01, masking=masked)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    name = "train8_kernel<cat,mask>" if masked else "train8_kernel<cat>"
    for it in range(2):
        u = rng.uniform(size=(T, E, A)).astype(np.float32)
        masks = random_masks(rng, T * E, A, special=False).reshape(T, E, A) if masked else np.ones((T, E, A), np.float32)
        ro = ref_rollout(ref, 500 + it, E, T, u, masks)
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        fields = ("obs", "actions", "values", "neglogp", "returns") + (("masks",) if masked else ())
        for f in fields:
            g.rollout_set(f, np.asarray(ro[f], np.float32))
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        k0 = g.kernel_counts()
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        d = delta(g.kernel_counts(), k0)
        if it == 0:                                              # the capture counts once, its replay does not
            assert d.get(name) == 8 and d.get("weight_grad_assemble_kernel") == 8, d
            assert "weight_grad_kernel" not in d and "grad_reduce_kernel" not in d and not any(k.startswith("train_fwd_bwd") for k in d), d
        else:
            assert name not in d and "weight_grad_assemble_kernel" not in d, d
        ref_rows, ref_mean = ref.update({f: np.asarray(ro[f], np.float32) for f in fields}, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    g.close()


@pytest.mark.gpu
def test_one_handle_through_changing_row_counts():
    """hazards this family has had before: a workspace or slot left over from a larger or smaller step must not reach the next one"""
    O, A = 18, 40
    ref, g = make(O, A, seed=2, ent_coef=0.01)
    for it, n in enumerate((100, 64, 256, 33, 100)):
        masked = it % 2 == 1
        mask = masks_for(n, A, 60 + it) if masked else None
        check_step(g, ref, synth_batch(ref, n, 70 + it, mask), mask, n, A, it, it)
    kc = g.kernel_counts()
    assert kc["train8_kernel<cat>"] == 3 and kc["train8_kernel<cat,mask>"] == 2 and kc["weight_grad_assemble_kernel"] == 5, kc
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_same_state_same_bits_also_behind_poisoned_lds(masked):
    """the same step twice from the same state gives the same bits; so does the step behind ppo_debug_poison_lds (a read of LDS the kernel never wrote would show)"""
    O, A, n = 36, 33, 100
    ref, g = make(O, A, seed=8, ent_coef=0.01)
    mask = masks_for(n, A, 1) if masked else None
    kw = {"mask": mask} if masked else {}
    g.train_step(LR, CR, *synth_batch(ref, 64, 20))             # non-zero Adam slots
    state = [g.get_flat(w) for w in range(3)]
    pw = g.beta_powers()
    batch = synth_batch(ref, n, 21, mask)
    outs = []
    for poison in (False, False, True):
        for w in range(3):
            g.set_flat(state[w], w)
        g.set_beta_powers(pw)
        if poison:
            g.debug_poison_lds()
        losses = g.train_step(LR, CR, *batch, **kw)
        outs.append([losses, g.last_grad()[0]] + [g.get_flat(w) for w in range(3)])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.isfinite(x).all()
            np.testing.assert_array_equal(x, y)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("switch,want", [("PPO_HIP_NO_T8", {"train_fwd_bwd_kernel<cat>": 1, "weight_grad_assemble_kernel": 1}),
                                         ("PPO_HIP_NO_DW2", {"train8_kernel<cat>": 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1})])
def test_switches_act_as_on_a_gaussian_handle(switch, want, monkeypatch):
    """PPO_HIP_NO_T8=1: the generic train kernel in front of weight_grad_assemble_kernel (a minibatch of whole 64-row chunks, as for a Gaussian handle);
    PPO_HIP_NO_DW2=1: train8_kernel<cat> in front of weight_grad_kernel + grad_reduce_kernel.  Both against the reference."""
    import ppo_cpp_amd
    O, A, n = 18, 18, 64
    monkeypatch.setenv(switch, "1")
    ref, g = make(O, A, seed=12, ent_coef=0.01)
    gauss = ppo_cpp_amd.PPOHip(O, A, list(HID))
    monkeypatch.delenv(switch)
    k0 = g.kernel_counts()
    check_step(g, ref, synth_batch(ref, n, 5), None, n, A, 0, 0)
    assert delta(g.kernel_counts(), k0) == want
    # the Gaussian handle created under the same switch takes the same two / three kernels (its own head's names)
    from tests import helpers as H
    from oracle import oracle as o
    orc = o.Oracle(O, A, list(HID)); orc.init_orthogonal(1)
    gauss.set_flat(orc.theta)
    mb = H.synth_minibatch(orc, n, seed=3)
    gauss.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    kg = {k: v for k, v in gauss.kernel_counts().items() if v}
    assert kg == {k.replace("<cat>", ""): v for k, v in want.items()}, kg
    g.close(); gauss.close()


@pytest.mark.gpu
def test_gates():
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import ACT_PAIR_KERNELS, PPOConfig
    from oracle import oracle as o
    from tests import helpers as H
    # flag + Gaussian: bitwise a plain Gaussian handle, same counts; ppo_action_dist reports the low bits only
    lib = ppo_cpp_amd.load_library()
    O, A, n = 18, 18, 100
    orc = o.Oracle(O, A, list(HID)); orc.init_orthogonal(1)
    mb = H.synth_minibatch(orc, n, seed=3)
    outs = []
    for flag in (0, ACT_PAIR_KERNELS):
        g = ppo_cpp_amd.PPOHip(O, A, list(HID), pair_kernels=bool(flag))          # (action_dist="gaussian": PPO_ACT_GAUSSIAN | PPO_ACT_PAIR_KERNELS)
        assert lib.ppo_action_dist(g.h) == 0
        g.set_flat(orc.theta)
        losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
        outs.append([losses, g.last_grad()[0], g.get_flat(0), g.get_flat(1), g.get_flat(2), {k: v for k, v in g.kernel_counts().items() if v}])
        g.close()
    for x, y in zip(outs[0][:5], outs[1][:5]):
        np.testing.assert_array_equal(x, y)
    assert outs[0][5] == outs[1][5] == {"train8_kernel": 1, "weight_grad_assemble_kernel": 1}, outs[0][5]
    # shapes that do not qualify: the generic categorical kernels, as without the flag (same bits)
    for O2, A2, hidden in ((18, 6, (64, 64)), (18, 6, (256, 256, 256)), (18, 65, (256, 256))):
        res = []
        for pair in (True, False):
            ref, g = make(O2, A2, hidden=hidden, seed=3, pair=pair)
            assert g.lib.ppo_action_dist(g.h) == 1
            losses = g.train_step(LR, CR, *synth_batch(ref, 48, 9))
            res.append([losses, g.get_flat(0), {k: v for k, v in g.kernel_counts().items() if v}])
            g.close()
        np.testing.assert_array_equal(res[0][0], res[1][0])
        np.testing.assert_array_equal(res[0][1], res[1][1])
        assert res[0][2] == res[1][2] == {"train_fwd_bwd_kernel<cat>": 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1}, (hidden, res[0][2])
    # the flag beside PPO_ACT_SHAPE_KERNELS on a narrow shape: the narrow family, as without it
    ref, g = make(18, 6, hidden=(64, 64), seed=3, shape_kernels=True)
    g.train_step(LR, CR, *synth_batch(ref, 48, 9))
    kc = {k: v for k, v in g.kernel_counts().items() if v}
    assert kc == {"narrow_train_kernel<cat>": 1}, kc
    g.close()
    # PPO_BF16: the flag changes nothing -- without PPO_ACT_BF16_HEAD the combination is still refused, with it the handle is created
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="categorical", pair_kernels=True, compute_dtype=1)
    gb = ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="categorical", pair_kernels=True, bf16_head=True, compute_dtype=1)
    gb.close()
    # an unknown distribution stays unknown beside the flag
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(256, 256)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    h = ctypes.c_void_p()
    assert lib.ppo_create_ex(ctypes.byref(cfg), ACT_PAIR_KERNELS | 2, ctypes.byref(h)) != 0
    assert b"unknown action_dist" in lib.ppo_last_error(None)
    # data parallel: refused with the documented message; the handle stays usable
    ref, g = make(18, 18, seed=1)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="data parallel is not supported for a categorical handle created with PPO_ACT_PAIR_KERNELS"):
        g.dist_init(1, 0, bytes(128))
    check_step(g, ref, synth_batch(ref, 32, 4), None, 32, 18, 0, 0)
    assert g.kernel_counts()["train8_kernel<cat>"] == 1
    g.close()


@pytest.mark.gpu
def test_ppo2_learns_the_discrete_target_task_on_the_pair():
    """tests/test_discrete_policy.test_ppo2_learns_the_discrete_target_task at hidden [256,256] with discrete_kernels="pair": DiscreteTargetEnv x 16, 64 steps,
    150 updates of 4 epochs x 4 minibatches through PPO2::learn.  A uniform policy earns 1/18 = 0.056.
    The NumPy reference loop (tests/categorical_ref.learn_loop on the same environment streams with the oracle's EnvNormalize, CatRef [256,256] from an orthogonal
    start with a 0.01 head, zero biases) over three draw seeds on the CPU, first-15 -> last-15 mean reward: 0.136 -> 0.504, 0.146 -> 0.497, 0.153 -> 0.484.  (The same
    loop at [64,64] gives 0.093 -> 0.429, inside the three figures tests/test_discrete_policy.py quotes for that width.)  The [64,64] task's lr 2e-3 learns at this
    width in the reference, so it is kept.
    RISE = 0.22: about two thirds of the smallest rise of the reference (0.331, 0.351, 0.368).
    BAND = 0.10 around REF_LAST15 = 0.495, the reference's mean over the seeds (they spread by 0.020, inside 0.10; the two legs differ in initial weights and draws).
    This leg on an MI355X: 0.125 -> 0.504."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15, LEARN_LR = 0.22, 0.10, 0.495, 2e-3
    got = hostapi.learn_curve(16, 64, [256, 256], 150, 4, 4, LEARN_LR, 0.2, seed=11, act_dim=18, discrete=True, discrete_kernels="pair")
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    kc = got["kernel_counts"]
    assert kc["train8_kernel<cat>"] > 0 and kc["weight_grad_assemble_kernel"] > 0 and kc["train_fwd_bwd_kernel<cat>"] == 0, kc
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
