"""Which train form serves which handle: the kernel_counts() deltas of ONE train_step and of ONE update (2 epochs) per case against
tests/golden/train_forms.json, recorded on the GPU from the commit named in that file (tools/record_train_forms.py) before the train / update host code
was reorganised.  The exact set of non-zero keys and their values must match: a handle that moves to another form, an extra or a missing launch all show here.

train_step: n rows drawn from a fixed RandomState, old values / neglogp from the handle's own step().  update: behind collect_synthetic(first=True), on-device
shuffle.  The data-parallel forms (all-reduce, bucketed, peer tiles, meeting Adam) are pinned by test_dp_two_ranks / test_dp_bench_flow / test_host_dp."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPOCHS = 2
GAMMA, LAM = 0.99, 0.95
CR, LR = 0.2, 3e-4
BF16 = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_forms.json")
SWITCHES = ("PPO_HIP_NO_NARROW_EPOCH", "PPO_HIP_NO_NARROW_EPOCH_XL", "PPO_HIP_NO_LAZY_ADAM", "PPO_HIP_NO_T8", "PPO_HIP_NO_DW2", "PPO_HIP_NO_REDUCE_ADAM",
            "PPO_HIP_ADAM_FAST", "PPO_HIP_NO_BF16_CHAIN")
UNSET = ("PPO_HIP_NO_NARROW", "PPO_HIP_NO_GRAPH", "PPO_HIP_NO_PEER_TILES", "PPO_HIP_NO_ADAM_MEET", "PPO_HIP_NO_ROLLOUT1", "PPO_HIP_NO_PERSISTENT_COLLECT")


NVEC = (3, 5, 4, 6)                                                    # the multi-categorical cases' components: sum = the A = 18 of every case


def case(hidden, O=18, A=18, E=16, T=4, nmb=2, n=128, env=(), dist="gaussian", shape_kernels=False, masking=False, bf16=False, pair_kernels=False, bf16_head=False):
    return dict(hidden=hidden, O=O, A=A, E=E, T=T, nmb=nmb, n=n, env=tuple(env), dist=dist, shape_kernels=shape_kernels, masking=masking, bf16=bf16,
                nvec=NVEC if dist == "multi_categorical" else None, pair_kernels=pair_kernels, bf16_head=bf16_head)


def bf16_case(env=(), **kw):
    return case((512, 512), O=64, E=64, T=8, nmb=4, env=env, bf16=True, **kw)


CASES = {
    # ---- narrow, static shape: the resident epoch launch, the deferred Adam, a launch per train step ----
    "nw_o18": case((64, 64)),
    "nw_o40": case((64, 64), O=40),                                    # the 64-column observation tile
    "nw_o18_no_epoch": case((64, 64), env=("PPO_HIP_NO_NARROW_EPOCH",)),
    "nw_o18_no_epoch_xl": case((64, 64), env=("PPO_HIP_NO_NARROW_EPOCH_XL",)),
    "nw_o18_no_lazy": case((64, 64), env=("PPO_HIP_NO_LAZY_ADAM",)),
    # ---- narrow, runtime shape (every padded width <= 64, but not [64,64]) ----
    "nw_runtime_32_32": case((32, 32)),
    # ---- narrow, categorical head ----
    "nw_cat": case((64, 64), dist="categorical", shape_kernels=True),
    "nw_cat_masking": case((64, 64), dist="categorical", shape_kernels=True, masking=True),
    # ---- the [256,256] pair ----
    "pair_n128": case((256, 256)),
    "pair_n100": case((256, 256), n=100),                              # padded to whole 64-row chunks
    "pair_no_t8_n128": case((256, 256), env=("PPO_HIP_NO_T8",)),
    "pair_no_t8_n100": case((256, 256), n=100, env=("PPO_HIP_NO_T8",)),     # not a whole number of chunks behind train_fwd_bwd_kernel: the generic path
    "pair_no_dw2": case((256, 256), env=("PPO_HIP_NO_DW2",)),
    # ---- fp32 generic ----
    "generic_o80": case((64, 64), O=80),                               # past the narrow family's 64 columns
    "generic_512_256_256": case((512, 256, 256)),
    # ---- categorical head on the generic path ----
    "cat_256": case((256, 256), dist="categorical"),
    "cat_256_masking": case((256, 256), dist="categorical", masking=True),
    # ---- bf16 ----
    "bf16": bf16_case(),
    "bf16_no_reduce_adam": bf16_case(env=("PPO_HIP_NO_REDUCE_ADAM",)),
    "bf16_adam_fast": bf16_case(env=("PPO_HIP_ADAM_FAST",)),
    "bf16_no_chain": bf16_case(env=("PPO_HIP_NO_BF16_CHAIN",)),
}
# ---- every head form of every family that has one, plain and with masking (recorded before the launch sites' head dispatch was gathered in one place) ----
for _m in (False, True):
    _s = "_masking" if _m else ""
    CASES.update({
        "mcat_256" + _s: case((256, 256), dist="multi_categorical", masking=_m),                                       # the generic fp32 family
        "pair_cat" + _s: case((256, 256), dist="categorical", pair_kernels=True, masking=_m),                          # the [256,256] pair
        "pair_mcat" + _s: case((256, 256), dist="multi_categorical", pair_kernels=True, masking=_m),
        "nw_mcat" + _s: case((64, 64), dist="multi_categorical", shape_kernels=True, masking=_m),                      # narrow
        "bf16_cat" + _s: bf16_case(dist="categorical", bf16_head=True, masking=_m),                                    # bf16
        "bf16_mcat" + _s: bf16_case(dist="multi_categorical", bf16_head=True, masking=_m),
    })


def set_switches(c, setenv, delenv):
    """every switch the train forms listen to, stated: the case's own set to 1, the others to 0"""
    for s in SWITCHES:
        setenv(s, "1" if s in c["env"] else "0")
    for s in UNSET:
        delenv(s)


def minibatch(g, c):
    """n train rows: observations and advantages from a fixed RandomState, actions / values / neglogp from the handle's own act model"""
    rng = np.random.RandomState(11)
    n, O, A = c["n"], c["O"], c["A"]
    obs = rng.normal(size=(n, O)).astype(np.float32)
    cat = c["dist"] != "gaussian"
    noise = rng.uniform(0.01, 0.99, (n, A)).astype(np.float32) if cat else rng.normal(size=(n, A)).astype(np.float32)
    mask = None
    if c["masking"]:
        mask = (rng.uniform(size=(n, A)) < 0.6).astype(np.float32); mask[:, 0] = 1.0
        if c["nvec"]:
            mask[:, np.cumsum(c["nvec"][:-1])] = 1.0                    # an open category in every component
    act, val, nlp = g.step(obs, noise, mask=mask)
    advs = rng.normal(size=n).astype(np.float32)
    returns = (val + rng.normal(size=n) * 0.1).astype(np.float32)
    return (obs, act, advs, returns, nlp, val), mask


def delta(before, after):
    return {k: int(after[k] - before.get(k, 0)) for k in after if after[k] != before.get(k, 0)}


def run_case(c):
    """{"train_step": delta, "update": delta} of kernel_counts(), non-zero entries only.  The switches are read from the environment: set_switches first."""
    import ppo_cpp_amd
    over = dict(compute_dtype=BF16) if c["bf16"] else {}
    g = ppo_cpp_amd.PPOHip(c["O"], c["A"], list(c["hidden"]), action_dist=c["dist"], shape_kernels=c["shape_kernels"], nvec=c["nvec"],
                           pair_kernels=c["pair_kernels"], bf16_head=c["bf16_head"], **over)
    try:
        g.init_orthogonal(0)
        if c["masking"]:
            g.set_action_masking(True)
        g.norm_init(c["E"], GAMMA); g.rollout_alloc(c["E"], c["T"]); g.seed(99)
        mb, mask = minibatch(g, c)
        deltas = {}
        before = g.kernel_counts()
        g.train_step(LR, CR, *mb, mask=mask)
        deltas["train_step"] = delta(before, g.kernel_counts())
        g.collect_synthetic(1234, GAMMA, LAM, None, env0=0, step0=0, first=True)
        before = g.kernel_counts()
        g.update(LR, CR, EPOCHS, c["nmb"], seed=5)
        deltas["update"] = delta(before, g.kernel_counts())
        return deltas
    finally:
        g.close()


def test_the_table_names_every_case():
    table = json.load(open(GOLDEN))
    assert table["epochs"] == EPOCHS and sorted(table["cases"]) == sorted(CASES)
    assert len(table["parent"]) == 40
    for name in CASES:
        assert sorted(table["cases"][name]) == ["train_step", "update"], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_train_form_kernel_counts(name, monkeypatch):
    want = json.load(open(GOLDEN))["cases"][name]
    set_switches(CASES[name], monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    got = run_case(CASES[name])
    print(name, got)
    assert got == want, (name, got, want)
