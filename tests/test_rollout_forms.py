"""Which rollout form serves which handle: the kernel_counts() delta of ONE rollout (T = 3) per case against tests/golden/rollout_forms.json,
recorded on the GPU from the commit named in that file (tools/record_rollout_forms.py) before the rollout host code was reorganised.  The exact set of
non-zero keys and their values must match: a handle that moves to another form, an extra or a missing launch all show here.

Device env: collect_synthetic(first=True).  Host Env: rollout_reset, then act / observe per step and finish, transitions from a fixed RandomState."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 3
GAMMA, LAM = 0.99, 0.95
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_forms.json")
SWITCHES = ("PPO_HIP_NO_ROLLOUT1", "PPO_HIP_NO_PERSISTENT_COLLECT", "PPO_HIP_NO_HOST_RESIDENT", "PPO_HIP_NO_HOST_FUSED", "PPO_HIP_NO_DIRECT_ACT")
UNSET = ("PPO_HIP_DIRECT_ACT_MAX_BLOCKS", "PPO_HIP_HOST_POLLS")


NVEC = (3, 5, 4, 6)                                                    # the multi-categorical cases' components: sum = the A = 18 of every case


def case(side, hidden, E, O=18, env=(), noise=False, dist="gaussian", masking=False, mask=False, shape_kernels=False, host_fused=False):
    return dict(side=side, hidden=hidden, E=E, O=O, env=tuple(env), noise=noise, dist=dist, masking=masking, mask=mask,
                nvec=NVEC if dist == "multi_categorical" else None, shape_kernels=shape_kernels, host_fused=host_fused)


CASES = {
    # ---- device env ----
    "dev_e1": case("dev", (64, 64), 1),
    "dev_e1_no_rollout1": case("dev", (64, 64), 1, env=("PPO_HIP_NO_ROLLOUT1",)),
    "dev_e8": case("dev", (64, 64), 8),
    "dev_e40": case("dev", (64, 64), 40),
    "dev_e96": case("dev", (64, 64), 96),
    "dev_e8_no_persistent": case("dev", (64, 64), 8, env=("PPO_HIP_NO_PERSISTENT_COLLECT",)),
    "dev_e96_no_persistent": case("dev", (64, 64), 96, env=("PPO_HIP_NO_PERSISTENT_COLLECT",)),
    "dev_256_e16": case("dev", (256, 256), 16),
    "dev_o80_e8": case("dev", (64, 64), 8, O=80),                      # past the 64-column limit: the general path
    # ---- host Env ----
    "host_e1": case("host", (64, 64), 1),
    "host_e8": case("host", (64, 64), 8),
    "host_e8_noise": case("host", (64, 64), 8, noise=True),
    "host_e8_no_resident": case("host", (64, 64), 8, env=("PPO_HIP_NO_HOST_RESIDENT",)),
    "host_e8_no_fused": case("host", (64, 64), 8, env=("PPO_HIP_NO_HOST_FUSED",)),
    "host_e40": case("host", (64, 64), 40),
    "host_e40_noise": case("host", (64, 64), 40, noise=True),
    "host_256_e16": case("host", (256, 256), 16),
    "host_256_e80": case("host", (256, 256), 80),                      # five row blocks: past the direct-publish limit of four
    "host_256_e16_no_direct": case("host", (256, 256), 16, env=("PPO_HIP_NO_DIRECT_ACT",)),
    "host_cat_masking_256_e16_mask": case("host", (256, 256), 16, dist="categorical", masking=True, mask=True),
    "host_cat_masking_256_e16_plain": case("host", (256, 256), 16, dist="categorical", masking=True),
}
# the head forms the table above does not reach (recorded before the launch sites' head dispatch was gathered in one place).  Kept apart from CASES:
# tests/test_counter_draws.py derives its rollouts from CASES, and its draw model knows the heads above only.
HEAD_CASES = {
    # ---- a multi-categorical [256,256] handle ----
    "dev_mcat_256_e16": case("dev", (256, 256), 16, dist="multi_categorical"),
    "host_mcat_256_e16": case("host", (256, 256), 16, dist="multi_categorical"),
}
# ---- host Env, set_host_step_fused on a narrow discrete handle: one launch per env step ----
for _d, _n in (("categorical", "cat"), ("multi_categorical", "mcat")):
    HEAD_CASES["host_fused_%s_e8" % _n] = case("host", (64, 64), 8, dist=_d, shape_kernels=True, host_fused=True)
    HEAD_CASES["host_fused_%s_e8_mask" % _n] = case("host", (64, 64), 8, dist=_d, shape_kernels=True, host_fused=True, masking=True, mask=True)
ALL_CASES = dict(CASES, **HEAD_CASES)

FIELDS = ("obs", "actions", "values", "neglogp", "rewards", "returns", "dones")


def set_switches(c, setenv, delenv):
    """every switch the forms listen to, stated: the case's own set to 1, the others to 0"""
    for s in SWITCHES:
        setenv(s, "1" if s in c["env"] else "0")
    for s in UNSET:
        delenv(s)


def run_case(c, rollouts=1, outputs=False):
    """(kernel_counts() delta of the first rollout, non-zero entries only; {name: array} of every rollout's fields and statistics when asked for).
    The switches are read from the environment: set_switches first."""
    import ppo_cpp_amd
    E, O, A = c["E"], c["O"], 18
    g = ppo_cpp_amd.PPOHip(O, A, list(c["hidden"]), action_dist=c["dist"], nvec=c["nvec"], shape_kernels=c["shape_kernels"])
    try:
        g.init_orthogonal(0)
        if c["host_fused"]:
            g.set_host_step_fused(True)
        if c["masking"]:
            g.set_action_masking(True)
        g.norm_init(E); g.rollout_alloc(E, T); g.seed(99)
        rng = np.random.RandomState(7)
        if c["side"] == "host":
            g.rollout_reset(rng.uniform(-1, 1, (E, O)).astype(np.float32))
        delta, got = None, {}
        for it in range(rollouts):
            before = g.kernel_counts()
            if c["side"] == "dev":
                g.collect_synthetic(1234, GAMMA, LAM, None, env0=0, step0=it * T, first=(it == 0))
            else:
                for t in range(T):
                    noise = rng.normal(size=(E, A)).astype(np.float32) if c["noise"] else None
                    if c["dist"] != "gaussian" and noise is not None:
                        noise = rng.uniform(0.01, 0.99, (E, A)).astype(np.float32)
                    mask = None
                    if c["mask"]:
                        mask = (rng.uniform(size=(E, A)) < 0.6).astype(np.float32); mask[:, 0] = 1.0
                        if c["nvec"]:
                            mask[:, np.cumsum(c["nvec"][:-1])] = 1.0    # an open category in every component
                    g.rollout_act(t, noise, mask=mask)
                    g.rollout_observe(t, rng.uniform(-1, 1, (E, O)).astype(np.float32), rng.uniform(-1, 1, E).astype(np.float32),
                                      (rng.uniform(size=E) < 0.1).astype(np.float32))
                g.rollout_finish(GAMMA, LAM)
            if it == 0:
                after = g.kernel_counts()
                delta = {k: int(after[k] - before.get(k, 0)) for k in after if after[k] != before.get(k, 0)}
            if outputs:
                for f in FIELDS + (("masks",) if c["masking"] else ()):
                    got["%s%d" % (f, it)] = g.rollout_get(f)
                for which, nm in ((0, "obs"), (1, "ret")):
                    m, v, cnt = g.norm_stats(which)
                    got["%s_mean%d" % (nm, it)], got["%s_var%d" % (nm, it)], got["%s_cnt%d" % (nm, it)] = m, v, np.float64(cnt)
        return delta, got
    finally:
        g.close()


def test_the_table_names_every_case():
    table = json.load(open(GOLDEN))
    assert table["T"] == T and sorted(table["cases"]) == sorted(ALL_CASES)
    assert len(table["parent"]) == 40


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_rollout_form_kernel_counts(name, monkeypatch):
    want = json.load(open(GOLDEN))["cases"][name]
    set_switches(ALL_CASES[name], monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    got, _ = run_case(ALL_CASES[name])
    print(name, got)
    assert got == want, (name, got, want)
