"""The one-launch host-Env step of the narrow discrete heads: ppo_set_host_step_fused / PPOHip.set_host_step_fused on a categorical or multi-categorical handle
created with PPO_ACT_SHAPE_KERNELS -> narrow_host_step_kernel<cat|mcat[,mask]> (csrc/ppo_narrow.hpp) against tests/multi_categorical_ref.py and against the
per-step form of the same handle.

The kernel is one workgroup of 32 rows (two pipes of 16); a lane owns the logit columns part + 16 k.  Shapes, the smallest at which it can go wrong:
E in {1, 5, 17, 32} (one live row and a dead second pipe; a ragged first pipe; a second pipe with one live row and, with K = 3, a 51-float action block; full),
T = 4 and TWO rollouts (the transition that is pending across rollout_finish, the state carried over).  Heads: 6 categories and the one component {18} on the
static shape; (3, 5, 2, 8): a component that crosses the 16-column lane boundary; sixteen components of 2: every lane stores an index; 64 categories: no padding
column, all four lane slots; (2, 17, 16, 5): 40 logits behind a 64-column observation tile; tiny runtime widths.

Which nets take the form.  The rule includes one_group_lds <= 160 KB: the handle's LDS image (both weight directions and the train tiles) plus the 13,472 bytes
of the fused step's state.  Behind [64,64] that holds for every action tile of 32 columns (about 140 KB with a 32-column observation tile, 155 KB with 64)
and for none of 64 columns (about 170 KB): (18, 64 categories, [64,64]) and (50, (2, 17, 16, 5), [64,64]) run the per-step form, silently -- they are cases of
the fallback test -- and the 64-column action tile is covered on the fused form behind [32,32] towers (about 105 / 115 KB), where the head code is the same.
Every fused case asserts through ppo_kernel_counts that the fused kernel is what ran.

Actions are compared on "clear" (row, component) pairs: those whose two best perturbed logits are more than 2 x LOGIT_TOL apart under the float64 reference
(tests/test_narrow_multi_discrete.py's rule); every parametrisation is checked on the CPU, from the reference alone, to have at least 0.9 of them.
The references of the categorical cases are MultiCatRef with one component, which is MaskedCatRef / CatRef expression for expression (checked below too).

Fused against per-step with normalisation off: both forms feed the raw observations, run nw_dense over the same tiles and the same head statements; the
test compares obs, actions and neglogp bitwise."""
import functools
import inspect
import os

import numpy as np
import pytest

from tests import counter_draws_ref as draws_ref
from tests import truncation_ref as tr
from tests.categorical_ref import CatRef
from tests.masked_categorical_ref import MaskedCatRef
from tests.masked_categorical_ref import random_masks as cat_random_masks
from tests.multi_categorical_ref import MultiCatRef, random_masks
from tests.test_multi_discrete import GAMMA, LAM, check_rollout, close, ref_rollout, upload_and_update
from tests.test_narrow_multi_discrete import LOGIT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("narrow_host_step<cat>", "narrow_host_step<cat,mask>", "narrow_host_step<mcat>", "narrow_host_step<mcat,mask>")
ES = [1, 5, 17, 32]
T = 4
FIELDS = ("obs", "actions", "values", "neglogp", "rewards", "returns", "dones")
# (observations, head, hidden): head an int = categorical with that many categories, a tuple = multi-categorical components
CAT, MCAT = (18, 6, (64, 64)), (18, (3, 5, 2, 8), (64, 64))
OTHER = [(7, 6, (4, 5)), (18, 64, (32, 32)), (50, 40, (32, 32)),
         (18, (2,) * 16, (64, 64)), (18, (18,), (64, 64)), (36, (6, 6, 6), (64, 64)), (50, (2, 17, 16, 5), (32, 32)), (7, (2, 3), (4, 5))]
REF_CASES = [(s, E) for s in (CAT, MCAT) for E in ES] + [(s, 17) for s in OTHER]
TOO_LARGE = [(18, 64, (64, 64)), (50, (2, 17, 16, 5), (64, 64))]         # one_group_lds > 160 KB: the per-step form
FORM_CASES = [(CAT, 5), (MCAT, 17), (MCAT, 32), ((7, (2, 3), (4, 5)), 1)]


def nvec_of(spec):
    return (spec[1],) if isinstance(spec[1], int) else tuple(spec[1])


def names_of(spec):
    """(fused, fused masked, per-step, per-step masked) names of ppo_kernel_counts for this head"""
    h = "cat" if isinstance(spec[1], int) else "mcat"
    return ("narrow_host_step<%s>" % h, "narrow_host_step<%s,mask>" % h, "narrow_step_kernel<%s>" % h, "narrow_step_kernel<%s,mask>" % h)


def case_seed(spec, E):
    return 100 * E + 7 * spec[0] + sum(nvec_of(spec)) + len(nvec_of(spec))


@functools.lru_cache(maxsize=None)
def reference(spec, seed, ent_coef=0.01):
    O, _, hidden = spec
    ref = MultiCatRef(O, nvec_of(spec), hidden, ent_coef=ent_coef)
    ref.init_random(seed)
    return ref


def counter_uniforms(seed, E, A, step):
    return draws_ref.counter_uniforms(draws_ref.seed_key(seed), np.arange(E), step, A).astype(np.float32)


def case_inputs(spec, E, masked, counter=None, n_roll=2):
    """(explicit uniforms [n_roll][T, E, A] -- or the counter draws of seed(counter) --, masks [n_roll][T, E, A] or None, env seed)"""
    A, nvec = sum(nvec_of(spec)), nvec_of(spec)
    rng = np.random.RandomState(case_seed(spec, E) + (1000 if masked else 0))
    if counter is None:
        us = [rng.uniform(size=(T, E, A)).astype(np.float32) for _ in range(n_roll)]
    else:
        us = [np.stack([counter_uniforms(counter, E, A, it * T + t) for t in range(T)]) for it in range(n_roll)]
    masks = [np.stack([random_masks(rng, E, nvec, special=True) for _ in range(T)]) for _ in range(n_roll)] if masked else None
    return us, masks, 99 + E


def ref_rollouts(ref, env_seed, E, us, masks=None, norm=True, dones=None):
    """tests/test_multi_discrete.ref_rollout continued over len(us) rollouts: the normaliser's state, the last observations and dones carried over.
    norm=False: the raw observations and rewards.  dones [n_roll * T, E]: in place of the seeded env's own."""
    from oracle import oracle as o
    from oracle import numpy_port as npp
    nz = o.Normalizer(E, ref.O)
    raw, _, _ = o.seeded_env_step(env_seed, 0, E, 0, ref.O)
    obs, d = (nz.obs(raw) if norm else raw), np.zeros(E, np.float32)
    k, out = 0, []
    for it, u in enumerate(us):
        ro = {f: [] for f in ("obs", "actions", "values", "neglogp", "dones", "rewards", "pert", "logits")}
        for t in range(len(u)):
            mk = None if masks is None else masks[it][t]
            a, v, nlp, pert = ref.step(obs, u[t], mk)
            for f, x in (("obs", obs), ("actions", a), ("values", v), ("neglogp", nlp), ("dones", d), ("pert", pert), ("logits", ref.forward(obs)[0])):
                ro[f].append(x)
            raw, rew, d = o.seeded_env_step(env_seed, 0, E, k + 1, ref.O)
            if dones is not None:
                d = dones[k]
            k += 1
            obs = nz.obs(raw) if norm else raw
            ro["rewards"].append(nz.reward(rew, d) if norm else rew)
        ro = {f: np.array(x) for f, x in ro.items()}
        _, last_v = ref.forward(obs)
        ro["returns"] = npp.gae(ro["rewards"].astype(np.float32), ro["values"].astype(np.float32), ro["dones"], last_v.astype(np.float32), d, GAMMA, LAM)
        if masks is not None:
            ro["masks"] = masks[it]
        out.append(ro)
    return out


def clear_of(ref, ros):
    """[n_roll][T, E, K] bool: the pairs whose two best perturbed logits (forbidden ones at -inf) are more than 2 LOGIT_TOL apart under the reference"""
    return [(ref.top2_gap(ro["pert"].reshape(-1, ref.A)) > 2 * LOGIT_TOL).reshape(ro["pert"].shape[:2] + (ref.K,)) for ro in ros]


@functools.lru_cache(maxsize=None)
def reference_case(spec, E, masked, counter=None, norm=True):
    us, masks, env_seed = case_inputs(spec, E, masked, counter)
    ref = reference(spec, case_seed(spec, E))
    ros = ref_rollouts(ref, env_seed, E, us, masks, norm)
    return ref, us, masks, env_seed, ros, clear_of(ref, ros)


def make_handle(spec, seed, fused=True, shape_kernels=True, masking=False, ent_coef=0.01):
    import ppo_cpp_amd
    O, head, hidden = spec
    if isinstance(head, int):
        g = ppo_cpp_amd.PPOHip(O, head, list(hidden), action_dist="categorical", shape_kernels=shape_kernels, ent_coef=ent_coef)
    else:
        g = ppo_cpp_amd.PPOHip(O, None, list(hidden), action_dist="multi_categorical", nvec=list(head), shape_kernels=shape_kernels, ent_coef=ent_coef)
    g.set_flat(reference(spec, seed, ent_coef).theta.astype(np.float32))
    if fused:
        g.set_host_step_fused(True)
    if masking:
        g.set_action_masking(True)
    return g


def drive(g, spec, E, env_seed, us=None, masks=None, n_roll=2, plain=False, dones=None, want_masks=False):
    """the host-Env loop over the seeded env, n_roll rollouts of T steps: [n_roll] dicts of every rollout field, the returned actions and the running statistics.
    us None: the handle's counter draws.  plain: rollout_act without a mask (on whatever handle)."""
    from oracle import oracle as o
    O, K = spec[0], len(nvec_of(spec))
    raw, _, _ = o.seeded_env_step(env_seed, 0, E, 0, O)
    g.rollout_reset(raw)
    k, out = 0, []
    for it in range(n_roll):
        acts = []
        for t in range(T):
            a = g.rollout_act(t, None if us is None else us[it][t], mask=None if (masks is None or plain) else masks[it][t])
            acts.append(a.reshape(E, K))
            raw, rew, d = o.seeded_env_step(env_seed, 0, E, k + 1, O)
            if dones is not None:
                d = dones[k]
            k += 1
            g.rollout_observe(t, raw, rew, d)
        g.rollout_finish(GAMMA, LAM)
        got = {f: g.rollout_get(f) for f in FIELDS}
        got["actions"] = got["actions"].reshape(T, E, K)
        got["returned"] = np.array(acts)
        if want_masks:
            got["masks"] = g.rollout_get("masks")
        for which, nm in ((0, "obs"), (1, "ret")):
            m, v, c = g.norm_stats(which)
            got[nm + "_mean"], got[nm + "_var"], got[nm + "_count"] = m, v, np.float64(c)
        out.append(got)
    return out


def start(g, E):
    g.norm_init(E)
    g.rollout_alloc(E, T)


def same_bits(a, b, msg):
    for x, y in zip(a, b):
        for f in x:
            np.testing.assert_array_equal(x[f], y[f], err_msg="%s: %s" % (msg, f))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "int ppo_set_host_step_fused(ppo_handle* h, int32_t on);" in src
    assert "int ppo_host_step_fused(const ppo_handle* h);" in src
    assert "#define PPO_ABI_VERSION 3" in src
    import ppo_cpp_amd
    lib = ppo_cpp_amd.load_library()
    assert hasattr(lib, "ppo_set_host_step_fused") and hasattr(lib, "ppo_host_step_fused")
    assert lib.ppo_abi_version() == 3
    for name in NEW:
        assert len(name) < 32           # ppo_kernel_counts' char[32]


def test_python_and_host_layers_carry_the_setting():
    import ppo_cpp_amd
    from ppo_cpp_amd import hostapi
    assert hostapi.HostArgs._fields_[-1][0] == "host_step_fused"
    assert inspect.signature(hostapi.learn_curve).parameters["host_step_fused"].default is False
    assert inspect.signature(hostapi.learn_masked).parameters["host_step_fused"].default is False
    assert callable(ppo_cpp_amd.PPOHip.set_host_step_fused) and isinstance(ppo_cpp_amd.PPOHip.host_step_fused, property)
    src = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo_host.cpp")).read()
    i = src.index("struct ppo_host_args {")
    assert src[i:src.index("};", i)].rstrip().splitlines()[-1].strip().startswith("int host_step_fused;")     # the struct's last member, as in HostArgs
    assert src.count("if (a->host_step_fused && ppo_set_host_step_fused(h, 1) != 0)") == 3                    # run_learn, the masked entry, the multi entry


def test_one_component_reference_is_the_categorical_reference():
    """the categorical cases are held to MultiCatRef with one component: the same actions and neglogp as CatRef / MaskedCatRef, to the last bit"""
    O, A, hidden, n = 18, 6, (64, 64), 40
    m = reference((O, A, hidden), 3)
    rng = np.random.RandomState(0)
    obs, u = rng.uniform(-1, 1, (n, O)), rng.uniform(size=(n, A))
    mask = cat_random_masks(rng, n, A, special=True)
    c, mc = CatRef(O, A, hidden), MaskedCatRef(O, A, hidden)
    c.theta, mc.theta = m.theta.copy(), m.theta.copy()
    a, _, nlp = c.step(obs, u)[:3]
    am, _, nlpm = m.step(obs, u)[:3]
    np.testing.assert_array_equal(am[:, 0], a); np.testing.assert_array_equal(nlpm, nlp)
    a, _, nlp = mc.step(obs, u, mask)[:3]
    am, _, nlpm = m.step(obs, u, mask)[:3]
    np.testing.assert_array_equal(am[:, 0], a); np.testing.assert_array_equal(nlpm, nlp)


def all_parametrisations():
    for spec, E in REF_CASES:
        for masked in (False, True):
            yield spec, E, masked, None, True
    for spec, E in FORM_CASES:
        for masked in (False, True):
            yield spec, E, masked, 5, True
            yield spec, E, masked, 5, False


def test_reference_alone_has_clear_margins_in_every_case():
    """the input condition of the action comparisons, from the float64 reference alone: in every parametrisation used below at least 0.9 of the (row, component)
    pairs are clear, and (check_rollout's own rule) none of them is a near-tie of 1e-5"""
    worst = 1.0
    for spec, E, masked, counter, norm in all_parametrisations():
        ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked, counter, norm)
        share = float(np.concatenate([c.reshape(-1) for c in clear]).mean())
        ties = sum(int((ref.top2_gap(ro["pert"].reshape(-1, ref.A)) < 1e-5).sum()) for ro in ros)
        worst = min(worst, share)
        assert share >= 0.9 and ties == 0, (spec, E, masked, counter, norm, share, ties)
        if masked:                                                  # the special rows are there: only the first / only the last category of every component
            off = np.concatenate([[0], np.cumsum(nvec_of(spec))])
            assert np.all(masks[0][0][0].nonzero()[0] == off[:-1]) and (E < 2 or np.all(masks[0][0][1].nonzero()[0] == off[1:] - 1))
    print("smallest share of clear pairs: %.4f" % worst)
    ro0 = ref_rollout(reference(MCAT, case_seed(MCAT, 5)), 99 + 5, 5, T, case_inputs(MCAT, 5, False)[0][0])      # the first rollout IS test_multi_discrete's
    mine = reference_case(MCAT, 5, False)[4][0]
    for f in ro0:
        np.testing.assert_array_equal(ro0[f], mine[f], err_msg=f)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def assert_fused_counts(kc, spec, acts, masked_acts, finishes, extra_value_passes=0):
    fu, fum, ps, psm = names_of(spec)
    assert kc[fu] == acts and kc[fum] == masked_acts, kc
    assert kc[ps] == 2 * finishes + extra_value_passes and kc[psm] == 0, kc       # per finish: the values of all rows, the bootstrap value
    for name, cnt in kc.items():
        if name not in (fu, fum, ps) and name.startswith(("narrow_", "policy_step_kernel", "bf16_step")):
            assert cnt == 0, (name, kc)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [CAT, MCAT])
@pytest.mark.parametrize("masked", [False, True])
def test_which_kernel_ran(spec, masked):
    E = 5
    ref, us, masks, env_seed, ros, _ = reference_case(spec, E, masked)
    fu, fum, ps, psm = names_of(spec)
    g = make_handle(spec, case_seed(spec, E), masking=masked)
    assert g.host_step_fused is True
    start(g, E)
    drive(g, spec, E, env_seed, us, masks, n_roll=1)
    assert_fused_counts(g.kernel_counts(), spec, 0 if masked else T, T if masked else 0, 1)
    g.close()
    g = make_handle(spec, case_seed(spec, E), fused=False, masking=masked)       # the setter off: today's counts
    assert g.host_step_fused is False
    start(g, E)
    drive(g, spec, E, env_seed, us, masks, n_roll=1)
    kc = g.kernel_counts()
    assert all(kc[n] == 0 for n in NEW), kc
    assert kc[psm if masked else ps] == T + (0 if masked else 1) and kc[ps] == (1 if masked else T + 1), kc
    g.close()


@pytest.mark.gpu
def test_settings_that_keep_todays_form(monkeypatch):
    import ppo_cpp_amd
    from oracle import oracle as o

    def counts_after_a_rollout(g, spec, E):
        start(g, E)
        drive(g, spec, E, 7, n_roll=1)
        kc = g.kernel_counts()
        g.close()
        assert all(kc[n] == 0 for n in NEW), kc
        return kc

    fu, fum, ps, psm = names_of(MCAT)
    kc = counts_after_a_rollout(make_handle(MCAT, 1), MCAT, 40)                   # more than one row group
    assert kc[ps] == T + 1, kc
    for spec in TOO_LARGE:                                                         # image + the step's state over 160 KB
        kc = counts_after_a_rollout(make_handle(spec, 1), spec, 5)
        assert kc[names_of(spec)[2]] == T + 1, kc
    kc = counts_after_a_rollout(make_handle(MCAT, 1, shape_kernels=False), MCAT, 5)      # not on the narrow family
    assert kc["policy_step_kernel<mcat>"] == T + 1 and kc[ps] == 0, kc
    # a Gaussian handle: its own forms, the same counts with and without the setting
    both = []
    for on in (False, True):
        g = ppo_cpp_amd.PPOHip(18, 18, [64, 64])
        g.set_host_step_fused(on)
        assert g.host_step_fused is on
        g.norm_init(5); g.rollout_alloc(5, T); g.seed(3)
        raw, _, _ = o.seeded_env_step(7, 0, 5, 0, 18)
        g.rollout_reset(raw)
        for t in range(T):
            g.rollout_act(t, None)
            g.rollout_observe(t, *o.seeded_env_step(7, 0, 5, t + 1, 18))
        g.rollout_finish(GAMMA, LAM)
        both.append((g.kernel_counts(), [g.rollout_get(f) for f in FIELDS]))
        g.close()
    assert both[0][0] == both[1][0] and all(both[1][0][n] == 0 for n in NEW), both[1][0]
    for x, y in zip(both[0][1], both[1][1]):
        np.testing.assert_array_equal(x, y)
    monkeypatch.setenv("PPO_HIP_NO_HOST_FUSED", "1")
    kc = counts_after_a_rollout(make_handle(MCAT, 1), MCAT, 5)
    assert kc[ps] == T + 1, kc


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("spec,E", REF_CASES)
def test_two_rollouts_and_two_updates_match_reference(spec, E, masked):
    ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked)
    g = make_handle(spec, case_seed(spec, E), masking=masked)
    start(g, E)
    got = drive(g, spec, E, env_seed, us, masks, want_masks=masked)
    assert_fused_counts(g.kernel_counts(), spec, 0 if masked else 2 * T, 2 * T if masked else 0, 2)
    share = float(np.concatenate([c.reshape(-1) for c in clear]).mean())
    print("pairs compared: %.4f" % share)
    assert share >= 0.9
    for it in range(2):
        msg = "rollout %d" % it
        np.testing.assert_array_equal(got[it]["actions"][clear[it]], ros[it]["actions"].astype(np.float32)[clear[it]], err_msg=msg)
        np.testing.assert_array_equal(got[it]["returned"], got[it]["actions"], err_msg=msg)
        np.testing.assert_array_equal(got[it]["dones"], ros[it]["dones"], err_msg=msg)
        if masked:
            np.testing.assert_array_equal(got[it]["masks"], masks[it], err_msg=msg)
            off = np.concatenate([[0], np.cumsum(nvec_of(spec))])[:-1]
            assert np.all(np.take_along_axis(masks[it], got[it]["actions"].astype(np.int64) + off, 2) != 0), "a forbidden category was sampled"
        check_rollout(ref, got[it], ros[it], msg)
    rng = np.random.RandomState(3)
    work = MultiCatRef(spec[0], nvec_of(spec), spec[2], ent_coef=0.01)           # (the update moves the reference's weights: not the shared one)
    work.theta = ref.theta.copy()
    for it in range(2):
        mk = [np.stack([random_masks(rng, E, nvec_of(spec)) for _ in range(T)])] if masked else None
        ro = ref_rollouts(work, 500 + it, E, [rng.uniform(size=(T, E, work.A)).astype(np.float32)], mk)[0]
        ro["obs"] = ro["obs"].astype(np.float32)
        upload_and_update(work, g, ro, rng, E, T, 2, 2, it)
    g.close()


@pytest.mark.gpu
def test_one_component_is_the_categorical_fused_handle_bit_for_bit():
    E = 17
    for masked in (False, True):
        us, masks, env_seed = case_inputs((18, 18, (64, 64)), E, masked)
        outs = []
        for spec in ((18, 18, (64, 64)), (18, (18,), (64, 64))):
            g = make_handle(spec, 4, masking=masked)
            g.set_flat(reference((18, 18, (64, 64)), 4).theta.astype(np.float32))
            start(g, E)
            outs.append(drive(g, spec, E, env_seed, us, masks, want_masks=masked))
            assert_fused_counts(g.kernel_counts(), spec, 0 if masked else 2 * T, 2 * T if masked else 0, 2)
            g.close()
        same_bits(outs[0], outs[1], "categorical vs one component, masked=%s" % masked)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [CAT, MCAT])
def test_all_ones_masks_and_the_plain_call_give_the_unmasked_bits_and_runs_repeat(spec):
    E = 17
    us, _, env_seed = case_inputs(spec, E, False)
    ones = [np.ones((T, E, sum(nvec_of(spec))), np.float32)] * 2
    outs = {}
    for form in ("unmasked", "again", "ones", "plain"):
        masking = form in ("ones", "plain")
        g = make_handle(spec, case_seed(spec, E), masking=masking)
        start(g, E)
        outs[form] = drive(g, spec, E, env_seed, us, ones if masking else None, plain=form == "plain", want_masks=masking)
        fu, fum, _, _ = names_of(spec)
        kc = g.kernel_counts()
        assert kc[fum] == (2 * T if form == "ones" else 0) and kc[fu] == (0 if form == "ones" else 2 * T), (form, kc)
        g.close()
    same_bits(outs["unmasked"], outs["again"], "the same case twice")
    for form in ("ones", "plain"):
        for it in range(2):
            np.testing.assert_array_equal(outs[form][it].pop("masks"), 1.0, err_msg=form)
        same_bits(outs["unmasked"], outs[form], form)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("spec,E", FORM_CASES)
def test_fused_against_the_per_step_form(spec, E, masked):
    """counter draws of one seed, the same transitions (dones of our own: one in seven), two rollouts"""
    dones = (np.random.RandomState(E).uniform(size=(2 * T, E)) < 1.0 / 7).astype(np.float32)
    for norm in (True, False):
        ref, us, masks, env_seed, ros, clear = reference_case(spec, E, masked, 5, norm)
        outs = []
        for fused in (True, False):
            g = make_handle(spec, case_seed(spec, E), fused=fused, masking=masked)
            start(g, E)
            g.norm_set_flags(norm, norm)
            g.seed(5)
            outs.append(drive(g, spec, E, env_seed, None, masks, dones=dones, want_masks=masked))
            kc = g.kernel_counts()
            assert (kc[names_of(spec)[1 if masked else 0]] == 2 * T) == fused, kc
            g.close()
        fu, st = outs
        share = float(np.concatenate([c.reshape(-1) for c in clear]).mean())
        assert share >= 0.9
        for it in range(2):
            msg = "norm=%s rollout %d: " % (norm, it)
            np.testing.assert_array_equal(fu[it]["dones"], st[it]["dones"], err_msg=msg + "dones")
            if masked:
                np.testing.assert_array_equal(fu[it]["masks"], st[it]["masks"], err_msg=msg + "masks")
            np.testing.assert_array_equal(fu[it]["actions"][clear[it]], st[it]["actions"][clear[it]], err_msg=msg + "actions")
            np.testing.assert_array_equal(fu[it]["actions"][clear[it]], ros[it]["actions"].astype(np.float32)[clear[it]], err_msg=msg + "actions (reference)")
            if not norm:
                for f in ("obs", "actions", "neglogp"):
                    np.testing.assert_array_equal(fu[it][f], st[it][f], err_msg=msg + f)
            same = np.all(fu[it]["actions"] == st[it]["actions"], axis=2)
            close(fu[it]["neglogp"][same], st[it]["neglogp"][same], rtol=2e-4, atol=2e-5, msg=msg + "neglogp")
            for f in ("obs", "values", "rewards", "returns", "obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count"):
                close(fu[it][f], st[it][f], rtol=2e-4, atol=2e-5, msg=msg + f)


@pytest.mark.gpu
def test_truncation_bootstrap_on_a_fused_handle():
    """tests/test_narrow_multi_discrete.test_truncation_bootstrap_uses_the_narrow_value_pass on a handle with the setting on"""
    spec, E, T6 = MCAT, 3, 6
    g = make_handle(spec, 9)
    ref = reference(spec, 9)
    rng = np.random.RandomState(12)
    step_dones = np.zeros((T6, E), np.float32)
    trunc = np.zeros((T6, E), bool)
    step_dones[2, 1] = 1.0; trunc[2, 1] = True                    # one marked row
    step_dones[4, 0] = 1.0                                        # and a real terminal state
    term_raw = rng.uniform(-1.5, 1.5, (T6, E, spec[0])).astype(np.float32)
    noise = rng.uniform(size=(T6, E, ref.A)).astype(np.float32)
    g.norm_init(E)
    g.rollout_alloc(E, T6)
    tr.host_rollout(g, 321, E, T6, step_dones, trunc, term_raw, GAMMA, LAM, noise)
    want = tr.ref_rollout(g, 321, E, T6, step_dones, trunc, term_raw, GAMMA, LAM)
    tv = g.rollout_get("terminal_values")
    close(g.rollout_get("values"), want["values"], rtol=2e-4, atol=2e-5, msg="values")
    close(tv[trunc], want["terminal_values"][trunc], rtol=2e-4, atol=2e-5, msg="terminal values")
    assert np.all(tv[~trunc] == 0.0) and abs(want["terminal_values"][2, 1]) > 1e-3
    close(g.rollout_get("returns"), want["returns"], rtol=2e-4, atol=2e-5, msg="returns")
    np.testing.assert_array_equal(g.rollout_get("dones")[1:], step_dones[:-1])
    kc = g.kernel_counts()
    assert kc["tval_scatter_kernel"] == 1, kc
    assert_fused_counts(kc, spec, T6, 0, 1, extra_value_passes=1)              # (the value-only pass over the marked row)
    g.close()


@pytest.mark.gpu
def test_a_refused_mask_launches_nothing_and_the_handle_goes_on():
    import ppo_cpp_amd
    spec, E = MCAT, 17
    ref, us, masks, env_seed, ros, clear = reference_case(spec, E, True)
    g = make_handle(spec, case_seed(spec, E), masking=True)
    start(g, E)
    from oracle import oracle as o
    g.rollout_reset(o.seeded_env_step(env_seed, 0, E, 0, spec[0])[0])
    bad = masks[0][0].copy(); bad[7, 3:8] = 0.0                   # component 1 of row 7 fully forbidden
    before = g.kernel_counts()
    with pytest.raises(ppo_cpp_amd.PPOHipError, match=r"row 7 allows no category of component 1"):
        g.rollout_act(0, us[0][0], mask=bad)
    assert g.kernel_counts() == before
    a = g.rollout_act(0, us[0][0], mask=masks[0][0])
    np.testing.assert_array_equal(a[clear[0][0]], ros[0]["actions"][0].astype(np.float32)[clear[0][0]])
    assert g.kernel_counts()["narrow_host_step<mcat,mask>"] == 1
    g.close()


@pytest.mark.gpu
def test_host_layer_runs_the_masked_multi_discrete_env_on_the_fused_step():
    from ppo_cpp_amd import hostapi
    run = lambda fused: hostapi.learn_curve(8, 16, [64, 64], 3, 4, 2, 2e-3, 0.2, seed=5, nvec=(6, 6, 6), masked=True, discrete_kernels="narrow",
                                            host_step_fused=fused, n_playback=30)
    got, was = run(True), run(False)
    kc, kc0 = got["kernel_counts"], was["kernel_counts"]
    assert got["forbidden_received"] == 0
    assert got["playback_actions"].shape == (30, 3) and np.all(got["playback_legal"] == 1.0)
    assert kc["narrow_host_step<mcat,mask>"] == 3 * 16 and all(kc0[n] == 0 for n in NEW), (kc, kc0)
    # acting counted nothing under the per-step name: what is left there is what the un-opted run counts besides its 48 act launches (the playback)
    assert kc["narrow_step_kernel<mcat,mask>"] == kc0["narrow_step_kernel<mcat,mask>"] - 3 * 16, (kc, kc0)
    assert kc["narrow_train_kernel<mcat,mask>"] == kc0["narrow_train_kernel<mcat,mask>"] > 0, (kc, kc0)


@pytest.mark.gpu
def test_ppo2_learns_the_discrete_target_task_on_the_fused_step():
    """tests/test_narrow_categorical.test_ppo2_learns_the_discrete_target_task_on_the_narrow_kernels with host_step_fused=True: its RISE / BAND / reference figure"""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.20, 0.10, 0.425
    got = hostapi.learn_curve(16, 64, [64, 64], 150, 4, 4, 2e-3, 0.2, seed=11, act_dim=18, discrete=True, discrete_kernels="narrow", host_step_fused=True)
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    kc = got["kernel_counts"]
    assert kc["narrow_host_step<cat>"] == 150 * 64 and kc["narrow_step_kernel<cat>"] == 2 * 150, kc
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
