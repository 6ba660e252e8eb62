"""The resident one-launch rollout of the narrow discrete heads: ppo_set_rollout_resident / PPOHip.set_rollout_resident on a categorical or multi-categorical
handle created with PPO_ACT_SHAPE_KERNELS -> the discrete overloads of narrow_rollout_kernel (csrc/ppo_narrow.hpp), on the device env (ppo_collect_synthetic) and
behind a host Env, against tests/multi_categorical_ref.py and against the per-step form of the same handle.

The kernel is one workgroup that walks the environments in groups of 32 rows (two pipes of 16); a lane owns the logit columns part + 16 k.  Environment counts,
the smallest at which it can go wrong: 1 (one live row, a dead second pipe), 5 (a ragged first pipe), 16 and 17 (the second pipe without and with one live
row), 32 (a full group), 33 (the MULTI instantiation, a second group with one live row), 64 (two full groups); T = 4 and TWO rollouts (the state carried over,
a transition pending across rollout_finish).  Heads and nets are tests/test_narrow_host_step.py's.

Behind a host Env the resident form serves steps WITHOUT explicit noise only, so the host-side comparisons draw with the counter generator (seed 5): the float64
reference gets the uniforms of tests/counter_draws_ref.py.  Actions are compared on "clear" (row, component) pairs (test_narrow_host_step.py's rule); the share of
clear pairs is checked on the CPU from the reference alone.  The two updates behind the two rollouts are test_narrow_host_step.py's (uploaded rollouts).

What is bitwise against the per-step form of the same handle (measured on an MI355X, see the tests):
  device env, normalisation on or off: every field -- obs, actions, neglogp, rewards, dones, the values of the batched pass, the returns --, both statistics with
  their counts and the carried state, over two rollouts, at every count.  A discrete handle's per-step form books a transition with norm_batch_kernel, which sums
  a batch's column in a fixed-shape tree; the discrete resident forms sum in that order (nw_chunk_moments_lds), not in the Gaussian resident kernel's sequential
  column loop, with which 36 of the 40 cases of test_device_env_is_bitwise_the_per_step_launches differed in the last bits;
  host Env, normalisation off: every field and the masks;
  host Env, normalisation on: held to the project's tolerances and to the float64 reference (a transition that a parked kernel left behind is booked by the
  bookkeeping-only launch of narrow_host_step_kernel, which sums in sequence)."""
import inspect
import os
import time

import numpy as np
import pytest

from tests import truncation_ref as tr
from tests.multi_categorical_ref import MultiCatRef, random_masks
from tests.test_multi_discrete import GAMMA, LAM, check_rollout, close, upload_and_update
from tests.test_narrow_host_step import (CAT, FIELDS, MCAT, T, case_inputs, case_seed, drive, make_handle, nvec_of, ref_rollouts, reference, reference_case,
                                         same_bits, start)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("narrow_rollout<cat>", "narrow_rollout<cat,mask>", "narrow_rollout<mcat>", "narrow_rollout<mcat,mask>")
ES = [1, 5, 16, 17, 32, 33, 64]
OTHER = [(18, (2,) * 16, (64, 64)), (50, 40, (32, 32)), (7, (2, 3), (4, 5))]
CASES = [(s, E) for s in (CAT, MCAT) for E in ES] + [(s, E) for s in OTHER for E in (17, 33)]
TOO_LARGE = (18, 64, (64, 64))                                     # the image + the rollout state over 160 KB
SEED = 5                                                           # the counter generator's seed behind a host Env
STATS = ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")


def names_of(spec):
    """(resident, resident masked, per-step, per-step masked, fused, fused masked) names of ppo_kernel_counts for this head"""
    h = "cat" if isinstance(spec[1], int) else "mcat"
    return tuple(n % h for n in ("narrow_rollout<%s>", "narrow_rollout<%s,mask>", "narrow_step_kernel<%s>", "narrow_step_kernel<%s,mask>",
                                 "narrow_host_step<%s>", "narrow_host_step<%s,mask>"))


def make(spec, seed, resident=True, fused=False, **kw):
    g = make_handle(spec, seed, fused=fused, **kw)
    if resident:
        g.set_rollout_resident(True)
    return g


def host_run(g, spec, E, env_seed, masks=None, us=None, n_roll=2, seed=SEED, norm=True, **kw):
    start(g, E)
    if not norm:
        g.norm_set_flags(False, False)
    g.seed(seed)
    return drive(g, spec, E, env_seed, us, masks, n_roll=n_roll, want_masks=masks is not None, **kw)


def dev_run(g, spec, E, env_seed, us=None, n_roll=2, norm=True):
    """n_roll rollouts on the device env (us: [n_roll][T, E, A] explicit uniforms, or None: the counter draws): every field and both statistics after each"""
    start(g, E)
    if not norm:
        g.norm_set_flags(False, False)
    out = []
    for it in range(n_roll):
        g.collect_synthetic(env_seed, GAMMA, LAM, None if us is None else us[it], step0=it * T, first=(it == 0))
        got = {f: g.rollout_get(f) for f in FIELDS}
        got["actions"] = got["actions"].reshape(T, E, -1)
        for which, nm in ((0, "obs"), (1, "ret")):
            m, v, c = g.norm_stats(which)
            got[nm + "_mean"], got[nm + "_var"], got[nm + "_count"] = m, v, np.float64(c)
        out.append(got)
    return out


def assert_resident_counts(kc, spec, launches, masked_launches, finishes, extra_value_passes=0):
    ro, rom, ps, psm = names_of(spec)[:4]
    assert kc[ro] == launches and kc[rom] == masked_launches, kc
    assert kc[ps] == 2 * finishes + extra_value_passes and kc[psm] == 0, kc       # per finish: the values of all rows, the bootstrap value
    for name, cnt in kc.items():
        if name not in (ro, rom, ps) and name.startswith(("narrow_", "policy_step_kernel", "bf16_step")):
            assert cnt == 0, (name, kc)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_set_rollout_resident(ppo_handle* h, int32_t on);" in src
    assert "int ppo_rollout_resident(const ppo_handle* h);" in src
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    assert hasattr(lib, "ppo_set_rollout_resident") and hasattr(lib, "ppo_rollout_resident")
    assert lib.ppo_abi_version() == 3
    for name in NEW:
        assert len(name) < 32           # ppo_kernel_counts' char[32]


def test_python_and_host_layers_carry_the_setting():
    import ppo_cpp_amd
    from ppo_cpp_amd import hostapi
    assert hostapi.HostArgs._fields_[-1][0] == "host_step_fused"                  # the struct keeps its layout: the setting travels beside it
    assert inspect.signature(hostapi.learn_curve).parameters["rollout_resident"].default is False
    assert inspect.signature(hostapi.learn_masked).parameters["rollout_resident"].default is False
    assert callable(ppo_cpp_amd.PPOHip.set_rollout_resident) and isinstance(ppo_cpp_amd.PPOHip.rollout_resident, property)
    src = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo_host.cpp")).read()
    assert "void ppo_host_set_rollout_resident(int on)" in src
    assert src.count("ppo_set_rollout_resident(h, 1) != 0") == 3                  # run_learn, the masked entry, the multi entry
    assert hasattr(hostapi.load_host_library(), "ppo_host_set_rollout_resident")
    assert "--resident_rollout" in open(os.path.join(ROOT, "ppo_cpp_amd", "host", "main.cpp")).read()


def all_parametrisations():
    for spec, E in CASES:
        for masked in (False, True):
            for counter in (None, SEED):
                for norm in (True, False):
                    yield spec, E, masked, counter, norm


def test_reference_alone_has_clear_margins_in_every_case():
    """the input condition of the action comparisons, from the float64 reference alone: in every parametrisation used below at least 0.9 of the (row, component)
    pairs are clear (the two best perturbed logits more than 2 LOGIT_TOL apart), and none of them is a near-tie of 1e-5"""
    worst = 1.0
    for spec, E, masked, counter, norm in all_parametrisations():
        ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked, counter, norm)
        share = float(np.concatenate([c.reshape(-1) for c in clear]).mean())
        ties = sum(int((ref.top2_gap(ro["pert"].reshape(-1, ref.A)) < 1e-5).sum()) for ro in ros)
        worst = min(worst, share)
        assert share >= 0.9 and ties == 0, (spec, E, masked, counter, norm, share, ties)
    print("smallest share of clear pairs: %.4f" % worst)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [CAT, MCAT])
@pytest.mark.parametrize("masked", [False, True])
def test_which_kernel_ran_behind_a_host_env(spec, masked):
    E = 5
    masks, env_seed = case_inputs(spec, E, masked, SEED)[1:]
    ro, rom, ps, psm = names_of(spec)[:4]
    g = make(spec, case_seed(spec, E), masking=masked)
    assert g.rollout_resident is True
    host_run(g, spec, E, env_seed, masks, n_roll=1)
    assert_resident_counts(g.kernel_counts(), spec, 0 if masked else 1, 1 if masked else 0, 1)
    g.close()
    g = make(spec, case_seed(spec, E), resident=False, masking=masked)            # the setter off: today's counts
    assert g.rollout_resident is False
    host_run(g, spec, E, env_seed, masks, n_roll=1)
    kc = g.kernel_counts()
    assert all(kc[n] == 0 for n in NEW), kc
    assert kc[psm if masked else ps] == T + (0 if masked else 1) and kc[ps] == (1 if masked else T + 1), kc
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [CAT, MCAT])
@pytest.mark.parametrize("E", [5, 40])
def test_which_kernel_ran_on_the_device_env(spec, E):
    for masking in (False, True):
        g = make(spec, case_seed(spec, E), masking=masking)
        dev_run(g, spec, E, 99 + E, n_roll=2)
        assert_resident_counts(g.kernel_counts(), spec, 2, 0, 2)                  # one launch per collect, the unmasked form on a masking handle too
        if masking:
            np.testing.assert_array_equal(g.rollout_get("masks"), 1.0)
        g.close()


def both_settings(build, run):
    """(counts, outputs) of run(build(resident)) with the setting off and on: the same counts, none of the new names, the same bits"""
    res = []
    for resident in (False, True):
        g = build(resident)
        assert g.rollout_resident is resident
        out = run(g)
        res.append((g.kernel_counts(), out))
        g.close()
    (kc0, out0), (kc1, out1) = res
    assert kc0 == kc1 and all(kc1[n] == 0 for n in NEW), (kc0, kc1)
    same_bits(out0, out1, "setting off vs on")
    return kc1


@pytest.mark.gpu
def test_settings_that_keep_todays_form(monkeypatch):
    import ppo_cpp_amd
    from oracle import oracle as o
    ps = names_of(MCAT)[2]
    host = lambda spec, E, **kw: (lambda g: host_run(g, spec, E, 7, n_roll=1, **kw))
    dev = lambda spec, E: (lambda g: dev_run(g, spec, E, 7, n_roll=1))
    mk = lambda spec, **kw: (lambda resident: make(spec, 1, resident=resident, **kw))
    # more than 64 environments
    assert both_settings(mk(MCAT), host(MCAT, 65))[ps] == T + 1
    assert both_settings(mk(MCAT), dev(MCAT, 65))[ps] == T + 1
    # the image plus the rollout state over 160 KB
    assert both_settings(mk(TOO_LARGE), host(TOO_LARGE, 5))[names_of(TOO_LARGE)[2]] == T + 1
    assert both_settings(mk(TOO_LARGE), dev(TOO_LARGE, 5))[names_of(TOO_LARGE)[2]] == T + 1
    # not on the narrow family
    kc = both_settings(mk(MCAT, shape_kernels=False), host(MCAT, 5))
    assert kc["policy_step_kernel<mcat>"] == T + 1 and kc[ps] == 0, kc
    both_settings(mk(MCAT, shape_kernels=False), dev(MCAT, 5))

    # a Gaussian handle: its own forms
    def gauss(resident):
        g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
        g.set_rollout_resident(resident)
        return g

    def gauss_run(g):
        g.norm_init(5); g.rollout_alloc(5, T); g.seed(3)
        g.rollout_reset(o.seeded_env_step(7, 0, 5, 0, 18)[0])
        for t in range(T):
            g.rollout_act(t, None)
            g.rollout_observe(t, *o.seeded_env_step(7, 0, 5, t + 1, 18))
        g.rollout_finish(GAMMA, LAM)
        out = {f: g.rollout_get(f) for f in FIELDS}
        g.collect_synthetic(7, GAMMA, LAM, None)
        out.update({"dev_" + f: g.rollout_get(f) for f in FIELDS})
        return [out]
    assert both_settings(gauss, gauss_run)["narrow_rollout_kernel"] == 2
    # explicit noise behind a host Env: the per-step form
    us = case_inputs(MCAT, 5, False)[0]
    assert both_settings(mk(MCAT), host(MCAT, 5, us=us))[ps] == T + 1
    # ... and with the fused setting on as well: the fused step
    g = make(MCAT, 1, fused=True)
    want = host_run(g, MCAT, 5, 7, us=us, n_roll=1)
    kc = g.kernel_counts(); g.close()
    assert kc["narrow_host_step<mcat>"] == T and all(kc[n] == 0 for n in NEW), kc
    g = make(MCAT, 1, resident=False, fused=True)
    same_bits(want, host_run(g, MCAT, 5, 7, us=us, n_roll=1), "explicit noise, fused: setting on vs off")
    g.close()
    # the switches
    monkeypatch.setenv("PPO_HIP_NO_PERSISTENT_COLLECT", "1")
    assert both_settings(mk(MCAT), dev(MCAT, 5))[ps] == T + 1
    monkeypatch.delenv("PPO_HIP_NO_PERSISTENT_COLLECT")
    for switch in ("PPO_HIP_NO_HOST_RESIDENT", "PPO_HIP_NO_HOST_FUSED"):
        monkeypatch.setenv(switch, "1")
        assert both_settings(mk(MCAT), host(MCAT, 5))[ps] == T + 1
        monkeypatch.delenv(switch)


def check_against_reference(spec, E, g, got, ros, clear, masks):
    share = float(np.concatenate([c.reshape(-1) for c in clear]).mean())
    print("pairs compared: %.4f" % share)
    assert share >= 0.9
    ref = reference(spec, case_seed(spec, E))
    for it in range(2):
        msg = "rollout %d" % it
        np.testing.assert_array_equal(got[it]["actions"][clear[it]], ros[it]["actions"].astype(np.float32)[clear[it]], err_msg=msg)
        if "returned" in got[it]:
            np.testing.assert_array_equal(got[it]["returned"], got[it]["actions"], err_msg=msg)
        np.testing.assert_array_equal(got[it]["dones"], ros[it]["dones"], err_msg=msg)
        if masks is not None:
            np.testing.assert_array_equal(got[it]["masks"], masks[it], err_msg=msg)
            off = np.concatenate([[0], np.cumsum(nvec_of(spec))])[:-1]
            assert np.all(np.take_along_axis(masks[it], got[it]["actions"].astype(np.int64) + off, 2) != 0), "a forbidden category was sampled"
        check_rollout(ref, got[it], ros[it], msg)
    rng = np.random.RandomState(3)
    work = MultiCatRef(spec[0], nvec_of(spec), spec[2], ent_coef=0.01)           # (the update moves the reference's weights: not the shared one)
    work.theta = ref.theta.copy()
    for it in range(2):
        mk = [np.stack([random_masks(rng, E, nvec_of(spec)) for _ in range(T)])] if masks is not None else None
        ro = ref_rollouts(work, 500 + it, E, [rng.uniform(size=(T, E, work.A)).astype(np.float32)], mk)[0]
        ro["obs"] = ro["obs"].astype(np.float32)
        upload_and_update(work, g, ro, rng, E, T, 2, 2, it)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("spec,E", CASES)
def test_host_env_two_rollouts_and_two_updates_match_reference(spec, E, masked):
    ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked, SEED)
    g = make(spec, case_seed(spec, E), masking=masked)
    got = host_run(g, spec, E, env_seed, masks)
    assert_resident_counts(g.kernel_counts(), spec, 0 if masked else 2, 2 if masked else 0, 2)
    check_against_reference(spec, E, g, got, ros, clear, masks)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spec,E", CASES)
def test_device_env_two_rollouts_and_two_updates_match_reference(spec, E):
    ref, us, _, env_seed, ros, clear = reference_case(spec, E, False)
    g = make(spec, case_seed(spec, E))
    got = dev_run(g, spec, E, env_seed, us)
    assert_resident_counts(g.kernel_counts(), spec, 2, 0, 2)
    check_against_reference(spec, E, g, got, ros, clear, None)
    g.close()


def dev_both_forms(spec, E, explicit, monkeypatch, norm):
    us = case_inputs(spec, E, False)[0] if explicit else None
    outs = []
    for resident in (True, False):
        monkeypatch.setenv("PPO_HIP_NO_PERSISTENT_COLLECT", "0" if resident else "1")
        g = make(spec, case_seed(spec, E))
        outs.append(dev_run(g, spec, E, 99 + E, us, norm=norm))
        assert (g.kernel_counts()[names_of(spec)[0]] == 2) == resident
        g.close()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("spec,E", CASES)
def test_device_env_is_bitwise_the_per_step_launches(spec, E, explicit, monkeypatch):
    """Normalisation on; every rollout field, both statistics with their counts and (the second collect) the carried state, resident against
    PPO_HIP_NO_PERSISTENT_COLLECT=1: the three-kernel path, whose norm_batch_kernel sums a batch in a tree.  The resident forms sum in that order; with the
    Gaussian resident kernel's sequential loop 36 of these 40 cases differed (largest difference of any field 2.9e-6, the actions equal in all)."""
    outs = dev_both_forms(spec, E, explicit, monkeypatch, True)
    for it in range(2):
        for f in outs[0][it]:
            a, b = np.asarray(outs[0][it][f]), np.asarray(outs[1][it][f])
            print("rollout %d, %s: %d of %d words differ, largest difference %.3g" % (it, f, int(np.sum(a != b)), a.size, float(np.max(np.abs(a - b)))))
    same_bits(outs[0], outs[1], "resident vs per-step")


@pytest.mark.gpu
@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("spec,E", CASES)
def test_device_env_without_normalisation_is_bitwise_the_per_step_launches(spec, E, explicit, monkeypatch):
    """the same with norm_set_flags(0, 0): every field (the values of the batched pass and the returns included), the carried state and both rollouts"""
    outs = dev_both_forms(spec, E, explicit, monkeypatch, False)
    same_bits(outs[0], outs[1], "normalisation off, resident vs per-step")


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("spec,E", CASES)
def test_host_env_against_the_per_step_form(spec, E, masked):
    """counter draws of one seed, the same transitions (dones of our own: one in seven), two rollouts.  Normalisation off: bitwise, the values of the batched
    pass and the returns included.  Normalisation on: the same actions on the clear pairs, everything else to the project's tolerances."""
    dones = (np.random.RandomState(E).uniform(size=(2 * T, E)) < 1.0 / 7).astype(np.float32)
    for norm in (False, True):
        ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked, SEED, norm)
        outs = []
        for resident in (True, False):
            g = make(spec, case_seed(spec, E), resident=resident, masking=masked)
            outs.append(host_run(g, spec, E, env_seed, masks, norm=norm, dones=dones))
            assert (g.kernel_counts()[names_of(spec)[1 if masked else 0]] == 2) == resident
            g.close()
        re, st = outs
        if not norm:
            same_bits(re, st, "normalisation off, resident vs per-step")
            continue
        for it in range(2):
            msg = "rollout %d: " % it
            np.testing.assert_array_equal(re[it]["dones"], st[it]["dones"], err_msg=msg + "dones")
            if masked:
                np.testing.assert_array_equal(re[it]["masks"], st[it]["masks"], err_msg=msg + "masks")
            np.testing.assert_array_equal(re[it]["actions"][clear[it]], st[it]["actions"][clear[it]], err_msg=msg + "actions")
            same = np.all(re[it]["actions"] == st[it]["actions"], axis=2)
            close(re[it]["neglogp"][same], st[it]["neglogp"][same], rtol=2e-4, atol=2e-5, msg=msg + "neglogp")
            for f in ("obs", "values", "rewards", "returns") + STATS:
                close(re[it][f], st[it][f], rtol=2e-4, atol=2e-5, msg=msg + f)


@pytest.mark.gpu
def test_one_component_is_the_categorical_resident_handle_bit_for_bit():
    E = 17
    for masked in (False, True):
        masks, env_seed = case_inputs((18, 18, (64, 64)), E, masked, SEED)[1:]
        host, dev = [], []
        for spec in ((18, 18, (64, 64)), (18, (18,), (64, 64))):
            g = make(spec, 4, masking=masked)
            g.set_flat(reference((18, 18, (64, 64)), 4).theta.astype(np.float32))
            host.append(host_run(g, spec, E, env_seed, masks))
            assert_resident_counts(g.kernel_counts(), spec, 0 if masked else 2, 2 if masked else 0, 2)
            dev.append(dev_run(g, spec, E, env_seed))
            g.close()
        same_bits(host[0], host[1], "host Env, categorical vs one component, masked=%s" % masked)
        same_bits(dev[0], dev[1], "device env, categorical vs one component, masking=%s" % masked)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [CAT, MCAT])
@pytest.mark.parametrize("E", [17, 33])
def test_all_ones_masks_and_the_plain_call_give_the_unmasked_bits_and_runs_repeat(spec, E):
    env_seed = 99 + E
    ones = [np.ones((T, E, sum(nvec_of(spec))), np.float32)] * 2
    outs = {}
    for form in ("unmasked", "again", "ones", "plain"):
        masking = form in ("ones", "plain")
        g = make(spec, case_seed(spec, E), masking=masking)
        outs[form] = host_run(g, spec, E, env_seed, ones if masking else None, plain=form == "plain")
        assert_resident_counts(g.kernel_counts(), spec, 0 if masking else 2, 2 if masking else 0, 2)      # a masking handle: the mask form, plain calls too
        g.close()
    same_bits(outs["unmasked"], outs["again"], "the same case twice")
    for form in ("ones", "plain"):
        for it in range(2):
            np.testing.assert_array_equal(outs[form][it].pop("masks"), 1.0, err_msg=form)
        same_bits(outs["unmasked"], outs[form], form)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_steps_with_and_without_explicit_noise_in_one_rollout(fused, monkeypatch):
    """a masking handle whose every other act brings explicit noise: the resident kernel is asked to leave, the transition it left is booked outside it, the step
    runs the per-step form (the fused one with that setting on as well) and the next act without noise relaunches the kernel -- the bits of the same handle
    without the resident setting, driven the same way (normalisation off)"""
    spec, E = MCAT, 5
    us, masks, env_seed = case_inputs(spec, E, True)
    monkeypatch.setenv("PPO_HIP_HOST_POLLS", "2000")
    outs = []
    for resident in (True, False):
        g = make(spec, case_seed(spec, E), resident=resident, fused=fused, masking=True)
        seq = [[u[t] if t % 2 else None for t in range(T)] for u in us]                 # drive() passes us[it][t]: no noise on the even steps
        outs.append(host_run(g, spec, E, env_seed, masks, us=seq, norm=False))
        kc = g.kernel_counts()
        ro, rom, ps, psm, fu, fum = names_of(spec)
        assert kc[rom] == (T if resident else 0) and kc[ro] == 0, kc                     # two rollouts, each: launched at step 0, relaunched at step 2
        assert kc[fum if fused else psm] == (T if resident else 2 * T), kc               # the steps with noise; without the setting: every step
        g.close()
    same_bits(outs[0], outs[1], "every other step with explicit noise, fused=%s" % fused)


def unruly(g, trans, masks, pauses):
    """test_hip_parity.test_resident_host_kernel_survives_an_unruly_host's script with masks; pauses: let the kernel's bounded waits run out (the resident leg)"""
    E, T10 = masks.shape[1], 10
    g.norm_init(E); g.rollout_alloc(E, T10); g.norm_set_flags(False, False); g.seed(7)
    pause = (lambda: time.sleep(0.05)) if pauses else (lambda: None)
    got = {}
    g.rollout_reset(trans[0][0]); k = 1; m = 0
    for t in range(4):                                               # an abandoned rollout
        got["a%d" % t] = g.rollout_act(t, None, mask=masks[m]); m += 1
        if t == 2:
            pause()                                                  # the kernel gives up waiting for the transition
        g.rollout_observe(t, *trans[k]); k += 1
        if t == 1:
            got["stats_mid"] = g.norm_stats(0)[0]                    # synchronises the stream while the kernel waits for the mask: it is asked to leave
            got["theta_mid"] = g.get_flat(0)
    g.rollout_reset(trans[k][0]); k += 1                             # start over
    for t in range(T10):
        if t == 3:
            pause()                                                  # between observe(t - 1) and act(t, mask): the kernel gives up waiting for the mask
        got["b%d" % t] = g.rollout_act(t, None, mask=masks[m]) if t != 5 else g.rollout_act(t, None); m += 1      # (one plain call: ones)
        g.rollout_observe(t, *trans[k]); k += 1
        if t == 6:
            got["value_mid"] = g.value(trans[0][0])                  # a policy evaluation in between (its own launches)
    g.rollout_finish(GAMMA, LAM)
    for f in FIELDS + ("masks",):
        got[f] = g.rollout_get(f)
    got["mean"], got["var"], cnt = g.norm_stats(0); got["cnt"] = np.float64(cnt)
    for t in range(3):                                               # a rollout that is finished early
        got["c%d" % t] = g.rollout_act(t, None, mask=masks[m]); m += 1
        g.rollout_observe(t, *trans[k]); k += 1
    g.rollout_finish(GAMMA, LAM)
    got["mean2"], got["var2"], cnt = g.norm_stats(0); got["cnt2"] = np.float64(cnt)
    got["rew_early"] = g.rollout_get("rewards")[:3]
    got["masks_early"] = g.rollout_get("masks")[:3]
    return got


@pytest.mark.gpu
def test_resident_discrete_kernel_survives_an_unruly_host(monkeypatch):
    """A masked multi-categorical handle whose host calls other entry points between observe and act (the kernel is asked to leave at its mask wait), pauses longer
    than the bounded waits (PPO_HIP_HOST_POLLS=2000: a few milliseconds; the kernel parks itself at the transition wait and at the mask wait and the next act
    relaunches it), evaluates the policy mid-rollout, abandons a rollout and finishes one early.  Every act result and every field: the bits of the per-step form
    driven the same way (normalisation off: a transition the parked kernel left is booked outside it, by a launch that sums in sequence).  The two pauses are 50 ms of host time, not a limit anything waits for."""
    spec, E = MCAT, 3
    rng = np.random.RandomState(3)
    trans = [(rng.uniform(-1, 1, (E, 18)).astype(np.float32), rng.uniform(-1, 1, E).astype(np.float32), (rng.uniform(size=E) < 0.2).astype(np.float32))
             for _ in range(40)]
    masks = np.stack([random_masks(rng, E, nvec_of(spec)) for _ in range(20)])
    monkeypatch.setenv("PPO_HIP_HOST_POLLS", "2000")
    outs = []
    for resident in (True, False):
        g = make(spec, 9, resident=resident, masking=True)
        outs.append(unruly(g, trans, masks, pauses=resident))
        kc = g.kernel_counts()
        g.close()
        if resident:
            # three rollouts, and a relaunch after each of: the stream synchronisation, the two pauses, the policy evaluation
            print("resident launches: %d" % kc["narrow_rollout<mcat,mask>"])
            assert kc["narrow_rollout<mcat,mask>"] >= 3 + 4 and kc["narrow_rollout<mcat>"] == 0, kc
            assert kc["narrow_step_kernel<mcat,mask>"] == 0, kc
        else:
            assert all(kc[n] == 0 for n in NEW), kc
    for key in outs[0]:
        np.testing.assert_array_equal(outs[0][key], outs[1][key], err_msg=key)


@pytest.mark.gpu
def test_a_refused_mask_launches_nothing_and_the_handle_goes_on():
    import ppo_cpp_amd
    from oracle import oracle as o
    spec, E = MCAT, 17
    ref, us, masks, env_seed, ros, clear = reference_case(spec, E, True, SEED)
    g = make(spec, case_seed(spec, E), masking=True)
    want = host_run(g, spec, E, env_seed, masks, n_roll=1)[0]       # the clean run
    g.close()
    g = make(spec, case_seed(spec, E), masking=True)
    start(g, E); g.seed(SEED)
    g.rollout_reset(o.seeded_env_step(env_seed, 0, E, 0, spec[0])[0])
    bad = masks[0][0].copy(); bad[7, 3:8] = 0.0                     # component 1 of row 7 fully forbidden
    for t in range(T):
        if t in (0, 2):                                             # before the first launch, and while the kernel waits for row 2's mask
            before = g.kernel_counts()
            with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
                g.rollout_act(t, None, mask=bad)
            assert g.kernel_counts() == before
        a = g.rollout_act(t, None, mask=masks[0][t])
        np.testing.assert_array_equal(a.reshape(E, -1), want["returned"][t])
        g.rollout_observe(t, *o.seeded_env_step(env_seed, 0, E, t + 1, spec[0]))
    g.rollout_finish(GAMMA, LAM)
    for f in FIELDS + ("masks",):
        np.testing.assert_array_equal(g.rollout_get(f).reshape(want[f].shape), want[f], err_msg=f)
    assert_resident_counts(g.kernel_counts(), spec, 0, 1, 1)
    g.close()


@pytest.mark.gpu
def test_truncation_bootstrap_on_a_resident_discrete_handle():
    """tests/test_narrow_host_step.test_truncation_bootstrap_on_a_fused_handle on a handle with the resident setting on (counter draws: no explicit noise)"""
    spec, E, T6 = MCAT, 3, 6
    g = make(spec, 9)
    rng = np.random.RandomState(12)
    step_dones = np.zeros((T6, E), np.float32)
    trunc = np.zeros((T6, E), bool)
    step_dones[2, 1] = 1.0; trunc[2, 1] = True                    # one marked row
    step_dones[4, 0] = 1.0                                        # and a real terminal state
    term_raw = rng.uniform(-1.5, 1.5, (T6, E, spec[0])).astype(np.float32)
    g.norm_init(E)
    g.rollout_alloc(E, T6)
    g.seed(SEED)
    tr.host_rollout(g, 321, E, T6, step_dones, trunc, term_raw, GAMMA, LAM, None)
    want = tr.ref_rollout(g, 321, E, T6, step_dones, trunc, term_raw, GAMMA, LAM)
    tv = g.rollout_get("terminal_values")
    close(g.rollout_get("values"), want["values"], rtol=2e-4, atol=2e-5, msg="values")
    close(tv[trunc], want["terminal_values"][trunc], rtol=2e-4, atol=2e-5, msg="terminal values")
    assert np.all(tv[~trunc] == 0.0) and abs(want["terminal_values"][2, 1]) > 1e-3
    close(g.rollout_get("returns"), want["returns"], rtol=2e-4, atol=2e-5, msg="returns")
    np.testing.assert_array_equal(g.rollout_get("dones")[1:], step_dones[:-1])
    kc = g.kernel_counts()
    assert kc["tval_scatter_kernel"] == 1, kc
    assert_resident_counts(kc, spec, 1, 0, 1, extra_value_passes=1)             # (the value-only pass over the marked row)
    g.close()


@pytest.mark.gpu
def test_host_layer_runs_the_masked_envs_on_the_resident_form():
    from ppo_cpp_amd import hostapi
    # the masked multi-discrete env (ppo_host_learn_multi)
    run = lambda resident: hostapi.learn_curve(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, nvec=(6, 6, 6), masked=True, discrete_kernels="narrow",
                                               rollout_resident=resident, n_playback=30)
    got, was = run(True), run(False)
    kc, kc0 = got["kernel_counts"], was["kernel_counts"]
    assert got["forbidden_received"] == 0
    assert got["playback_actions"].shape == (30, 3) and np.all(got["playback_legal"] == 1.0)
    # one launch per rollout (more only if the host was held up for longer than the kernel's bounded wait) and no act under the per-step name: what is left there
    # is what the un-opted run counts besides its 48 act launches (the playback)
    assert 3 <= kc["narrow_rollout<mcat,mask>"] < 3 * 16 and all(kc0[n] == 0 for n in NEW), (kc, kc0)
    assert kc["narrow_step_kernel<mcat,mask>"] == kc0["narrow_step_kernel<mcat,mask>"] - 3 * 16, (kc, kc0)
    assert kc["narrow_train_kernel<mcat,mask>"] == kc0["narrow_train_kernel<mcat,mask>"] > 0, (kc, kc0)
    # the masked categorical env (ppo_host_learn_masked); the default is cleared again behind either call
    got = hostapi.learn_masked(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, act_dim=6, discrete_kernels="narrow", rollout_resident=True)
    kc = got["kernel_counts"]
    assert got["forbidden_received"] == 0
    assert 3 <= kc["narrow_rollout<cat,mask>"] < 3 * 16 and kc["narrow_step_kernel<cat,mask>"] == 0, kc
    was = hostapi.learn_masked(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, act_dim=6, discrete_kernels="narrow")
    assert all(was["kernel_counts"][n] == 0 for n in NEW) and was["kernel_counts"]["narrow_step_kernel<cat,mask>"] == 3 * 16, was["kernel_counts"]


@pytest.mark.gpu
def test_ppo2_learns_the_discrete_target_task_on_the_resident_form():
    """tests/test_narrow_host_step.test_ppo2_learns_the_discrete_target_task_on_the_fused_step with rollout_resident=True: its sizes, its RISE / BAND / reference figure"""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.20, 0.10, 0.425
    got = hostapi.learn_curve(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, discrete=True, discrete_kernels="narrow", rollout_resident=True)
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    kc = got["kernel_counts"]
    assert 150 <= kc["narrow_rollout<cat>"] < 150 * 64 and kc["narrow_step_kernel<cat>"] == 2 * 150, kc
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
