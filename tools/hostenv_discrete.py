"""Host-Env rollout of the narrow discrete heads, small environment counts: us per env step of the act / observe loop (free env: constant transitions, counter
draws, T = 256, the first rollout discarded) for the per-step form ("general"), the one-launch form (ppo_set_host_step_fused, "fused", at most 32 environments)
and the resident form (ppo_set_rollout_resident, "resident", at most 64) of a categorical handle (18, 18, [64,64]; --categories N: another width), the same under
random half-open masks, a multi-categorical one (18, (6, 6, 6), [64,64]) and the latter under masks, every leg in a fresh child process.
usage: python tools/hostenv_discrete.py [--rounds N] [--categories N] [E ...]      (default: 3 alternating rounds, E = 1 8 32; PPO_HIP_LIBRARY selects another
build for the general legs: a build without a setter skips that setter's legs)"""
import os, sys, time, subprocess
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
HEADS = {"cat": dict(act_dim=18, action_dist="categorical"), "cat,mask": dict(act_dim=18, action_dist="categorical"),
         "mcat": dict(act_dim=None, action_dist="multi_categorical", nvec=[6, 6, 6]),
         "mcat,mask": dict(act_dim=None, action_dist="multi_categorical", nvec=[6, 6, 6])}
SETTER = {"fused": "ppo_set_host_step_fused", "resident": "ppo_set_rollout_resident"}
COUNTED = {"fused": "narrow_host_step<", "resident": "narrow_rollout<"}
if len(sys.argv) > 1 and sys.argv[1] == "--one":
    import ctypes as C, ppo_cpp_amd
    head, form, E, cats, T = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), 256
    kw = dict(HEADS[head]); act_dim = kw.pop("act_dim")
    if act_dim is not None: act_dim = cats
    g = ppo_cpp_amd.PPOHip(18, act_dim, [64, 64], shape_kernels=True, **kw); g.init_orthogonal(0)
    if form in SETTER:
        if not hasattr(g.lib, SETTER[form]): print("-"); sys.exit(0)
        if form == "fused": g.set_host_step_fused(True)
        else: g.set_rollout_resident(True)
    masked = head.endswith("mask")
    if masked: g.set_action_masking(True)
    g.norm_init(E, 0.99); g.rollout_alloc(E, T)
    A = g.A
    rng = np.random.RandomState(0)
    obs = rng.uniform(-1, 1, (E, 18)).astype(np.float32); rew = rng.uniform(-1, 1, E).astype(np.float32); dn = np.zeros(E, np.float32)
    mask = (rng.uniform(size=(E, A)) < 0.5).astype(np.float32); mask[:, ::6] = 1.0           # the first category of every component stays allowed
    K = 1 if head.startswith("cat") else 3
    act = np.zeros((E, K), np.float32); fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    g._ck(g.lib.ppo_rollout_reset(g.h, fp(obs)))
    tot = 0.0; n = 0
    for it in range(4):
        t0 = time.perf_counter()
        for t in range(T):
            if masked: g._ck(g.lib.ppo_rollout_act_masked(g.h, t, None, fp(mask), fp(act)))
            else: g._ck(g.lib.ppo_rollout_act(g.h, t, None, fp(act)))
            g._ck(g.lib.ppo_rollout_observe(g.h, t, fp(obs), fp(rew), fp(dn)))
        t1 = time.perf_counter()
        g._ck(g.lib.ppo_rollout_finish(g.h, C.c_float(0.99), C.c_float(0.95)))
        if it >= 1: tot += t1 - t0; n += T
    kc = g.kernel_counts()
    for f, prefix in COUNTED.items():                             # the leg measured the form it names
        assert (sum(c for k, c in kc.items() if k.startswith(prefix)) > 0) == (form == f), kc
    print("%.1f" % (1e6 * tot / n))
    sys.exit(0)
args = sys.argv[1:]
rounds, cats = 3, 18
while args and args[0] in ("--rounds", "--categories"):
    if args[0] == "--rounds": rounds = int(args[1])
    else: cats = int(args[1])
    args = args[2:]
for E in [int(x) for x in args] or [1, 8, 32]:
    for head in HEADS:
        got = {"general": [], "fused": [], "resident": []}
        if E > 32: del got["fused"]                                # (one row group: beyond it the setting does not take effect)
        for r in range(rounds):                                    # alternating: general, fused, resident, general, ...
            for form in got:
                out = subprocess.run([sys.executable, __file__, "--one", head, form, str(E), str(cats)], capture_output=True, text=True, timeout=120)
                if out.returncode != 0 or not out.stdout.strip():   # a leg that failed ends the run: nothing more is started on the device
                    sys.exit("E = %d %s %s failed (status %d):\n%s" % (E, head, form, out.returncode, out.stderr[-2000:]))
                got[form].append(out.stdout.strip().split("\n")[-1])
        print("E = %2d %-9s: " % (E, head) + " | ".join("%s %s us" % (form, " ".join(v)) for form, v in got.items()), flush=True)
