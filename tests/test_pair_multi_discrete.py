"""The multi-categorical head (and action masks) in the [256,256] kernel pair: ppo_create_multi_ex(cfg, nvec, K, PPO_ACT_PAIR_KERNELS) /
PPOHip(action_dist="multi_categorical", nvec=.., pair_kernels=True) runs train8_kernel<mcat[,mask]> + weight_grad_assemble_kernel instead of the generic four launches.

Reference: the float64 MultiCatRef of tests/multi_categorical_ref.py.  Tolerances: those of tests/test_pair_categorical.py for the same quantity (losses rtol 1e-4 /
atol 1e-6, clipfrac within one row, gradient rtol 2e-4 with atol 2e-6 of the largest element -- 4e-6 where sum(nvec) > 32 --, norm, weights, Adam m and v as there).
Hidden [256,256] is fixed by the kernel; every other size is the smallest that reaches the code.  train8_kernel gives a row 32 lanes, lane j owning logit columns j and
j + 32, so the shapes are one per instantiation <KP0, AP> and hazard: odd offsets; the 64-column observation tile; a component that runs across column 32 (lanes that
hold two of its columns, lanes that hold one column each of two components); the full tile with K = 16; A = 33, where only lane 0's second element is live and belongs
to the last component.  Rows 100 and 16: a last live tile with dead rows inside plus a dead tile, and one live tile with three dead ones behind it."""
import os

import numpy as np
import pytest

from tests.masked_categorical_ref import random_masks as cat_random_masks
from tests.multi_categorical_ref import MultiCatRef, offsets, random_masks
from tests.test_multi_discrete import make as make_multi
from tests.test_multi_discrete import ref_rollout, synth_batch
from tests.test_pair_categorical import CR, HID, LR, close, delta, padded_logstd_region

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(18, (3, 5, 2, 8)),          # <32,32>, odd offsets
          (36, (6, 6, 6)),             # <64,32>
          (18, (7, 30, 3)),            # <32,64>; component 1 spans columns 7..36: lanes 7..31 and 0..4 hold two of its columns, lanes 5..6 one each of components 1 and 2
          (50, (4,) * 16),             # <64,64>, the full tile, K = 16
          (18, (16, 17))]              # A = 33: only lane 0's second element is live, and it belongs to the last component
STRADDLE = (18, (7, 30, 3))
PAIR_KERNELS = 0x400
NEW = ("train8_kernel<mcat>", "train8_kernel<mcat,mask>")
REFUSAL = "data parallel is not supported for a multi-categorical handle created with PPO_ACT_PAIR_KERNELS"


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_states_the_names_and_the_refusal_and_keeps_the_abi():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ABI_VERSION 3" in src and "#define PPO_ACT_PAIR_KERNELS 0x400" in src
    assert '"train8_kernel<mcat>"' in src and '"train8_kernel<mcat,mask>"' in src
    assert REFUSAL in src
    assert "A multi-categorical handle has no such kernels" not in src
    for name in NEW:
        assert len(name) < 32           # ppo_kernel_counts' char[32]


class RecordingLib:
    """the real library with the two multi-categorical constructors replaced: they record their arguments and fail, so no device is looked for"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ppo_create_multi_ex(self, cfg, nvec, K, flags, out):
        self.calls.append(("ppo_create_multi_ex", [int(nvec[k]) for k in range(K)], int(flags)))
        return -1

    def ppo_create_multi(self, cfg, nvec, K, out):
        self.calls.append(("ppo_create_multi", [int(nvec[k]) for k in range(K)], 0))
        return -1

    def ppo_last_error(self, h):
        return b"recorded"


@pytest.mark.parametrize("kw,flags", [({}, 0), ({"pair_kernels": True}, 0x400), ({"shape_kernels": True}, 0x100), ({"shape_kernels": True, "pair_kernels": True}, 0x500),
                                      ({"pair_kernels": True, "bf16_head": True}, 0x400)])
def test_ppohip_forwards_pair_kernels_on_the_multi_branch(kw, flags, monkeypatch):
    import ppo_cpp_amd
    from ppo_cpp_amd import capi
    assert capi.ACT_PAIR_KERNELS == PAIR_KERNELS
    rec = RecordingLib(ppo_cpp_amd.load_library())
    monkeypatch.setattr(capi, "load_library", lambda *a, **k: rec)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="recorded"):
        ppo_cpp_amd.PPOHip(18, None, [256, 256], action_dist="multi_categorical", nvec=[7, 30, 3], **kw)
    assert len(rec.calls) == 1 and rec.calls[0][1:] == ([7, 30, 3], flags), rec.calls
    assert "pair_kernels=True with it" in ppo_cpp_amd.PPOHip.__doc__


def test_host_layers_name_the_pair():
    import inspect
    from ppo_cpp_amd import hostapi
    assert hostapi._discrete_kernels("generic") == 0 and hostapi._discrete_kernels("narrow") == 1 and hostapi._discrete_kernels("pair") == 2
    with pytest.raises(ValueError, match="discrete_kernels"):
        hostapi._discrete_kernels("wide")
    assert inspect.signature(hostapi.learn_curve).parameters["discrete_kernels"].default == "generic"
    main = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "main.cpp")).read()
    assert "--discrete_kernels narrow|pair|generic" in main and "expected narrow, pair or generic" in main
    assert "--discrete_kernels narrow|pair|generic" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    host = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo_host.cpp")).read()
    assert "nothing for a multi-discrete Env" not in host


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, nvec, hidden=HID, seed=0, pair=True, masking=False, **overrides):
    ref, g = make_multi(O, nvec, hidden, seed=seed, pair_kernels=pair, **overrides)
    if masking:
        g.set_action_masking(True)
    return ref, g


def nonzero(kc):
    return {k: v for k, v in kc.items() if v}


def masks_for(n, nvec, seed, dead=None):
    """random masks whose first rows allow only the first / only the last category of every component (a row whose action is its component's only allowed category);
    dead: that column is forbidden in EVERY row and its right neighbour (the same component) always allowed"""
    mask = random_masks(np.random.RandomState(seed), n, nvec)
    if dead is not None:
        mask[:, dead] = 0.0
        mask[:, dead + 1] = 1.0
    return mask


def check_step(g, ref, batch, mask, n, it, steps_so_far):
    """one train step of `g` against the same step of `ref`: losses, clipfrac within one row, gradient, clipped norm, weights, both Adam slots"""
    losses = g.train_step(LR, CR, *batch, mask=mask)
    grad, norm = g.last_grad()
    ref_losses, ref_grad = ref.train_step(LR, CR, *batch, mask=mask)
    print("it %d losses %s ref %s" % (it, losses, ref_losses))
    close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
    assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
    gs = np.abs(ref_grad).max()
    atol_g = (4e-6 if ref.A > 32 else 2e-6) * gs
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
@pytest.mark.parametrize("O,nvec", SHAPES)
def test_three_train_steps_match_reference(O, nvec, n, masked):
    ref, g = make(O, nvec, seed=9, ent_coef=0.01)
    dead = int(offsets(nvec)[1])                           # masked: the first category of component 1 is forbidden in EVERY row
    o_w, s_w = ref.offs["pi/w"]
    o_b, _ = ref.offs["pi/b"]
    k0 = g.kernel_counts()
    for it in range(3):
        mask = masks_for(n, nvec, 200 + it, dead) if masked else None
        batch = synth_batch(ref, n, 100 + it, mask=mask)
        if masked:
            single = np.stack([ref.comp(mask, k).sum(1) == 1 for k in range(ref.K)], 1)
            assert single.any() and np.all(np.take_along_axis(mask, batch[1].astype(np.int64) + offsets(nvec)[:-1], 1) != 0)
        _, grad = check_step(g, ref, batch, mask, n, it, it)
        if masked:
            gw = grad[o_w:o_w + s_w[0] * s_w[1]].reshape(s_w)
            assert np.all(gw[:, dead] == 0.0) and grad[o_b + dead] == 0.0, "the forbidden category's column / bias entry must get an exactly zero gradient"
            assert np.any(gw[:, :dead] != 0.0) and np.any(gw[:, dead + 1:] != 0.0)
    assert delta(g.kernel_counts(), k0) == {NEW[1] if masked else NEW[0]: 3, "weight_grad_assemble_kernel": 3}
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("A", [18, 40])
def test_one_component_is_the_flagged_categorical_handle_bit_for_bit(A):
    import ppo_cpp_amd
    O, n = 18, 100
    ref, gm = make(O, [A], seed=2, ent_coef=0.01)
    gc = ppo_cpp_amd.PPOHip(O, A, list(HID), action_dist="categorical", pair_kernels=True, ent_coef=0.01)
    gc.set_flat(ref.theta.astype(np.float32))
    rmask = cat_random_masks(np.random.RandomState(3), n, A)
    for mask in (None, rmask):
        for it in range(2):
            obs, a, adv, ret, nlp, v = synth_batch(ref, n, 30 + it, mask=mask)
            lm = gm.train_step(LR, CR, obs, a, adv, ret, nlp, v, mask=mask)
            lc = gc.train_step(LR, CR, obs, a[:, 0], adv, ret, nlp, v, mask=mask)
            assert np.isfinite(lm).all()
            np.testing.assert_array_equal(lm, lc)
            (g1, n1), (g2, n2) = gm.last_grad(), gc.last_grad()
            np.testing.assert_array_equal(g1, g2)
            assert n1 == n2
            for which in (0, 1, 2):
                np.testing.assert_array_equal(gm.get_flat(which), gc.get_flat(which))
    km, kc = gm.kernel_counts(), gc.kernel_counts()
    assert km[NEW[0]] == 2 and km[NEW[1]] == 2 and km["train8_kernel<cat>"] == 0 and km["train8_kernel<cat,mask>"] == 0, km
    assert kc["train8_kernel<cat>"] == 2 and kc["train8_kernel<cat,mask>"] == 2 and kc[NEW[0]] == 0 and kc[NEW[1]] == 0, kc
    gm.close(); gc.close()


@pytest.mark.gpu
def test_all_ones_masks_give_the_unmasked_bits():
    O, nvec = STRADDLE
    n = 100
    ref, g0 = make(O, nvec, seed=4, ent_coef=0.01)
    _, g1 = make(O, nvec, seed=4, ent_coef=0.01)
    ones = np.ones((n, ref.A), np.float32)
    for it in range(2):
        batch = synth_batch(ref, n, 11 + it)
        np.testing.assert_array_equal(g0.train_step(LR, CR, *batch), g1.train_step(LR, CR, *batch, mask=ones))
        for x, y in zip(g0.last_grad(), g1.last_grad()):
            np.testing.assert_array_equal(x, y)
        for which in range(3):
            np.testing.assert_array_equal(g0.get_flat(which), g1.get_flat(which))
    kc0, kc1 = g0.kernel_counts(), g1.kernel_counts()
    assert kc0[NEW[0]] == 2 and kc0[NEW[1]] == 0, kc0
    assert kc1[NEW[1]] == 2 and kc1[NEW[0]] == 0, kc1
    g0.close(); g1.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_flagged_against_unflagged(masked):
    """the method of tests/test_pair_categorical.test_flagged_against_unflagged"""
    O, nvec = STRADDLE
    n, A = 100, sum(nvec)
    ref, gp = make(O, nvec, seed=6, ent_coef=0.01)
    _, gg = make(O, nvec, seed=6, ent_coef=0.01, pair=False)
    off, width, size = padded_logstd_region(O, A)
    before = {k: gp.debug_buffer(k).view(np.float32).copy() for k in ("theta", "adam_m", "adam_v")}
    assert before["theta"].size == size
    # every padding element of the vector (the logstd region among them): where a flat vector of ones does not land
    _, probe = make(O, nvec, seed=6)
    probe.set_flat(np.ones(probe.P, np.float32))
    pad = probe.debug_buffer("theta").view(np.float32) != 1.0
    probe.close()
    assert pad[off:off + width].all() and pad.sum() == size - gp.P
    rng = np.random.RandomState(5)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = rng.uniform(size=(n, A)).astype(np.float32)
    mask = masks_for(n, nvec, 3) if masked else None
    for x, y in zip(gp.step(obs, u, mask=mask), gg.step(obs, u, mask=mask)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(gp.act_deterministic(obs, mask=mask), gg.act_deterministic(obs, mask=mask))
    for it in range(3):
        batch = synth_batch(ref, n, 40 + it, mask=mask)
        lp, lg = gp.train_step(LR, CR, *batch, mask=mask), gg.train_step(LR, CR, *batch, mask=mask)
        close(lp[:4], lg[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(lp[4] - lg[4]) <= 1.0 / n + 1e-6
        (grp, np_), (grg, ng) = gp.last_grad(), gg.last_grad()
        close(grp, grg, rtol=2e-4, atol=4e-6 * np.abs(grg).max(), msg="grad it=%d" % it)
        close(np_, ng, rtol=1e-4, msg="norm")
        close(gp.get_flat(0), gg.get_flat(0), rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
    kp, kg = gp.kernel_counts(), gg.kernel_counts()
    name = "<mcat,mask>" if masked else "<mcat>"
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
    (O, nvec), E, T, nmb, epochs = STRADDLE, 16, 16, 4, 2
    ref, g = make(O, nvec, seed=17, ent_coef=0.01, masking=masked)
    A = ref.A
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    name = NEW[1] if masked else NEW[0]
    for it in range(2):
        u = rng.uniform(size=(T, E, A)).astype(np.float32)
        masks = random_masks(rng, T * E, nvec, special=False).reshape(T, E, A) if masked else None
        ro = ref_rollout(ref, 500 + it, E, T, u, masks)
        assert ro["actions"].shape == (T, E, len(nvec))
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
    """a workspace, slot or action row left over from a larger or smaller step must not reach the next one"""
    O, nvec = STRADDLE
    ref, g = make(O, nvec, seed=2, ent_coef=0.01)
    for it, n in enumerate((100, 64, 256, 33, 100)):
        mask = masks_for(n, nvec, 60 + it) if it % 2 == 1 else None
        check_step(g, ref, synth_batch(ref, n, 70 + it, mask=mask), mask, n, it, it)
    kc = g.kernel_counts()
    assert kc[NEW[0]] == 3 and kc[NEW[1]] == 2 and kc["weight_grad_assemble_kernel"] == 5, kc
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("O,nvec", [STRADDLE, (36, (16, 17))])
def test_same_state_same_bits_also_behind_poisoned_lds(O, nvec, masked):
    """the same step twice from the same state gives the same bits; so does the step behind ppo_debug_poison_lds (a read of LDS the kernel never wrote would show)"""
    n = 100
    ref, g = make(O, nvec, seed=8, ent_coef=0.01)
    mask = masks_for(n, nvec, 1) if masked else None
    g.train_step(LR, CR, *synth_batch(ref, 64, 20))             # non-zero Adam slots
    state = [g.get_flat(w) for w in range(3)]
    pw = g.beta_powers()
    batch = synth_batch(ref, n, 21, mask=mask)
    outs = []
    for poison in (False, False, True):
        for w in range(3):
            g.set_flat(state[w], w)
        g.set_beta_powers(pw)
        if poison:
            g.debug_poison_lds()
        losses = g.train_step(LR, CR, *batch, mask=mask)
        outs.append([losses, g.last_grad()[0]] + [g.get_flat(w) for w in range(3)])
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.isfinite(x).all()
            np.testing.assert_array_equal(x, y)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("switch,want", [("PPO_HIP_NO_T8", {"train_fwd_bwd_kernel<mcat>": 1, "weight_grad_assemble_kernel": 1}),
                                         ("PPO_HIP_NO_DW2", {"train8_kernel<mcat>": 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1})])
def test_switches_act_as_on_a_flagged_categorical_handle(switch, want, masked, monkeypatch):
    """PPO_HIP_NO_T8=1: the generic train kernel in front of weight_grad_assemble_kernel (a minibatch of whole 64-row chunks);
    PPO_HIP_NO_DW2=1: train8_kernel<mcat[,mask]> in front of weight_grad_kernel + grad_reduce_kernel.  Both against the reference."""
    O, nvec, n = 18, (6, 6, 6), 64
    monkeypatch.setenv(switch, "1")
    ref, g = make(O, nvec, seed=12, ent_coef=0.01)
    monkeypatch.delenv(switch)
    mask = masks_for(n, nvec, 8) if masked else None
    k0 = g.kernel_counts()
    check_step(g, ref, synth_batch(ref, n, 5, mask=mask), mask, n, 0, 0)
    assert delta(g.kernel_counts(), k0) == {(k.replace("<mcat>", "<mcat,mask>") if masked else k): v for k, v in want.items()}
    g.close()


@pytest.mark.gpu
def test_gates():
    import ppo_cpp_amd
    generic = {"train_fwd_bwd_kernel<mcat>": 1, "weight_grad_kernel": 1, "grad_reduce_kernel": 1}
    # shapes that do not qualify: the generic <mcat> kernels, as without the flag (same bits)
    for O, nvec, hidden in ((18, (3, 3), (64, 64)), (18, (3, 3), (256, 256, 256)), (18, (2, 17, 16, 17, 13), (256, 256))):
        res = []
        for pair in (True, False):
            ref, g = make(O, nvec, hidden=hidden, seed=3, pair=pair)
            assert g.lib.ppo_action_dist(g.h) == 2
            losses = g.train_step(LR, CR, *synth_batch(ref, 48, 9))
            res.append([losses, g.last_grad()[0], g.get_flat(0), g.get_flat(1), g.get_flat(2), nonzero(g.kernel_counts())])
            g.close()
        for x, y in zip(res[0][:5], res[1][:5]):
            np.testing.assert_array_equal(x, y)
        assert res[0][5] == res[1][5] == generic, (hidden, res[0][5])
    # both flags: each acts where its own rule holds
    ref, g = make(18, (3, 3), hidden=(64, 64), seed=3, shape_kernels=True)
    g.train_step(LR, CR, *synth_batch(ref, 48, 9))
    assert nonzero(g.kernel_counts()) == {"narrow_train_kernel<mcat>": 1}, g.kernel_counts()
    g.close()
    ref, g = make(18, (3, 3), seed=3, shape_kernels=True)
    check_step(g, ref, synth_batch(ref, 48, 9), None, 48, 0, 0)
    assert nonzero(g.kernel_counts()) == {NEW[0]: 1, "weight_grad_assemble_kernel": 1}, g.kernel_counts()
    g.close()
    # PPO_BF16 stays refused
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, None, [256, 256], action_dist="multi_categorical", nvec=[3, 3], pair_kernels=True, compute_dtype=1)
    # data parallel: refused with the documented message; the handle stays usable
    ref, g = make(18, (6, 6, 6), seed=1)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=REFUSAL):
        g.dist_init(1, 0, bytes(128))
    check_step(g, ref, synth_batch(ref, 32, 4), None, 32, 0, 0)
    assert g.kernel_counts()[NEW[0]] == 1
    g.close()
    # an unflagged [256,256] handle still counts only the generic names
    ref, g = make(18, (6, 6, 6), seed=1, pair=False)
    g.train_step(LR, CR, *synth_batch(ref, 64, 4))
    assert nonzero(g.kernel_counts()) == generic, g.kernel_counts()
    g.close()


@pytest.mark.gpu
def test_ppo2_learns_the_multi_discrete_target_task_on_the_pair():
    """tests/test_multi_discrete.test_ppo2_learns_the_multi_discrete_target_task at hidden [256,256] with discrete_kernels="pair": MultiDiscreteTargetEnv x 16
    (nvec = (6, 6, 6)), 64 steps, N = 80 updates of 4 epochs x 4 minibatches at lr 2e-3 through PPO2::learn.  A uniform policy earns 1/6 = 0.167.
    The NumPy reference loop (tests/multi_categorical_ref.learn_loop on MultiDiscreteTargetRef(1234, 16, 18, nvec) with the oracle's EnvNormalize, MultiCatRef [256,256],
    init_random(seed, pi_gain=0.01)) over the draw seeds 1, 2, 3 on the CPU, first-15 -> last-15 mean reward: 0.209 -> 0.437, 0.210 -> 0.440, 0.231 -> 0.460.  (The
    same script at [64,64], seed 1, gives the 0.201 -> 0.406 that tests/test_multi_discrete.py quotes.)  N and lr are the [64,64] task's: the reference alone clears
    the margin with them at this width (after 60 updates its smallest rise is 0.178, after 120 it is 0.283).
    RISE = 0.152: two thirds of the smallest rise of the reference (0.2275, 0.2298, 0.2290).
    BAND = 0.094 around REF_LAST15 = 0.446, the reference's mean over the seeds: 4 x their spread (0.0235), the rule of the [64,64] test; the two legs differ in
    initial weights and draws.
    This leg on an MI355X: 0.223 -> 0.472 (rise 0.249; 0.026 from the reference mean)."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15, N, LEARN_LR = 0.152, 0.094, 0.446, 80, 2e-3
    got = hostapi.learn_curve(16, 64, [256, 256], N, 4, 4, LEARN_LR, 0.2, seed=11, nvec=(6, 6, 6), discrete_kernels="pair")
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    kc = got["kernel_counts"]
    assert kc["train8_kernel<mcat>"] > 0 and kc["weight_grad_assemble_kernel"] > 0 and kc["train_fwd_bwd_kernel<mcat>"] == 0, kc
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
