"""ctypes binding of libppo_host.so: the C++ host layer (Env stack, Runner, PPO2) above the libppo_hip C-ABI."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class HostArgs(C.Structure):
    _fields_ = [("n_envs", C.c_int), ("n_steps", C.c_int), ("n_hidden", C.c_int), ("hidden", C.c_int * 8),
                ("nminibatches", C.c_int), ("noptepochs", C.c_int), ("n_updates", C.c_int),
                ("lr", C.c_float), ("cliprange", C.c_float), ("gamma", C.c_float), ("lam", C.c_float),
                ("seeded_env", C.c_int), ("device", C.c_int), ("max_workers", C.c_int), ("reference_loop", C.c_int),
                ("norm_obs", C.c_int), ("norm_reward", C.c_int), ("seed", C.c_ulonglong), ("obs_dim", C.c_int), ("act_dim", C.c_int),
                ("cliprange_vf", C.c_float), ("discrete_kernels", C.c_int), ("compute_dtype", C.c_int),
                ("n_components", C.c_int), ("nvec", C.c_int * 16), ("multi_masked", C.c_int), ("host_step_fused", C.c_int)]


def _discrete_kernels(name):
    """ppo_host_args::discrete_kernels: 0 = the generic categorical kernels, 1 = PPO_ACT_SHAPE_KERNELS, 2 = PPO_ACT_PAIR_KERNELS, 3 = PPO_ACT_BINARY_SHAPE_KERNELS,
    4 = PPO_ACT_BINARY_PAIR_KERNELS (3 and 4: a multi-binary Env's handle: ppo_host_learn_binary, ppo_host_binary_checkpoint_ex; every other entry treats them as 0)"""
    if name not in ("generic", "narrow", "pair", "binary_narrow", "binary_pair"):
        raise ValueError("discrete_kernels must be 'generic', 'narrow', 'pair', 'binary_narrow' or 'binary_pair', not %r" % (name,))
    return {"generic": 0, "narrow": 1, "pair": 2, "binary_narrow": 3, "binary_pair": 4}[name]


class HostResult(C.Structure):
    _fields_ = [("env_steps_per_s", C.c_double), ("collect_ms", C.c_double), ("update_ms", C.c_double),
                ("losses", C.c_float * 5), ("fps_last", C.c_int), ("error", C.c_char * 256),
                ("obs_count", C.c_double), ("ret_count", C.c_double),
                ("phase_env_ms", C.c_double), ("phase_act_ms", C.c_double), ("phase_observe_ms", C.c_double),
                ("pool_workers", C.c_int), ("pool_chunk", C.c_int), ("pool_active", C.c_int)]


def load_host_library(build=True):
    global _LIB
    if _LIB is None:
        so = os.path.join(_PKG, "libppo_host.so")
        if build and os.path.exists("/opt/rocm/bin/hipcc"):
            from . import build as _b
            _b.build_hip()
            so = _b.build_host()
        C.CDLL(os.path.join(_PKG, "libppo_hip.so"), mode=C.RTLD_GLOBAL)
        _LIB = C.CDLL(so)
    return _LIB


def learn(n_envs, n_steps, hidden, n_updates, nminibatches=32, noptepochs=10, lr=3.93141e-4, cliprange=0.161023, gamma=0.99,
          lam=0.95, seeded_env=True, device=-1, max_workers=0, reference_loop=False, norm_obs=True, norm_reward=True, seed=0, obs_dim=18, act_dim=18,
          cliprange_vf=-1.0):
    """cliprange_vf: PPO2's value clipping: < 0 (the default) clips the value with cliprange, a finite value >= 0 with its own range, inf switches it off"""
    lib = load_host_library()
    a = HostArgs()
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.seeded_env, a.device, a.max_workers, a.reference_loop = int(seeded_env), device, max_workers, int(reference_loop)
    a.norm_obs, a.norm_reward, a.seed = int(norm_obs), int(norm_reward), seed
    a.obs_dim, a.act_dim = obs_dim, act_dim
    a.cliprange_vf = cliprange_vf
    r = HostResult()
    if lib.ppo_host_learn(C.byref(a), C.byref(r)) != 0:
        raise RuntimeError(r.error.decode())
    return {"env_steps_per_s": r.env_steps_per_s, "collect_ms": r.collect_ms, "update_ms": r.update_ms,
            "losses": [float(x) for x in r.losses], "fps_last": r.fps_last, "obs_count": r.obs_count, "ret_count": r.ret_count,
            "phase_ms": {"env_step": r.phase_env_ms, "act_kernel_d2h_sync": r.phase_act_ms, "observe_pack_h2d_enqueue": r.phase_observe_ms},
            "vec_env_pool": {"workers": r.pool_workers, "chunk": r.pool_chunk, "active_in_last_step": r.pool_active}}


class HostExplicit(C.Structure):
    _fields_ = [("theta_in", C.c_void_p), ("noise", C.c_void_p), ("perms", C.c_void_p), ("losses_out", C.c_void_p), ("theta_out", C.c_void_p),
                ("obs_mean", C.c_void_p), ("obs_var", C.c_void_p), ("obs_count", C.c_void_p),
                ("ret_mean", C.c_void_p), ("ret_var", C.c_void_p), ("ret_count", C.c_void_p), ("reward_curve", C.c_void_p),
                ("count_names", C.c_void_p), ("counts", C.c_void_p), ("n_counts", C.c_void_p), ("applied_out", C.c_void_p), ("target_kl", C.c_float)]


def learn_explicit(n_envs, n_steps, hidden, theta, noise, perms, nminibatches, lr=3.93141e-4, cliprange=0.161023, gamma=0.99, lam=0.95,
                   reference_loop=False, device=-1, obs_dim=18, act_dim=18, cliprange_vf=-1.0):
    """PPO2::learn for perms.shape[0] updates with explicit weights, exploration noise [U,T,E,A] and epoch permutations [U,epochs,B]
    on SeededEnvMock x n_envs behind VecEnv + EnvNormalize.  Returns per-update mean losses [U,5], final weights, obs_rms, ret_rms."""
    import numpy as np
    lib = load_host_library()
    U, epochs, B = perms.shape
    assert noise.shape[:3] == (U, n_steps, n_envs) and B == n_envs * n_steps
    theta = np.ascontiguousarray(theta, np.float32); noise = np.ascontiguousarray(noise, np.float32); perms = np.ascontiguousarray(perms, np.int32)
    a = HostArgs()
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, epochs, U
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.seeded_env, a.device, a.max_workers, a.reference_loop = 1, device, 0, int(reference_loop)
    a.norm_obs, a.norm_reward, a.seed = 1, 1, 0
    a.obs_dim, a.act_dim = obs_dim, act_dim
    a.cliprange_vf = cliprange_vf
    assert noise.shape[3] == act_dim
    out = {"losses": np.zeros((U, 5), np.float32), "theta": np.zeros(theta.size, np.float32),
           "obs_mean": np.zeros(obs_dim, np.float32), "obs_var": np.zeros(obs_dim, np.float32), "obs_count": np.zeros(1, np.float64),
           "ret_mean": np.zeros(1, np.float32), "ret_var": np.zeros(1, np.float32), "ret_count": np.zeros(1, np.float64)}
    x = HostExplicit(theta.ctypes.data, noise.ctypes.data, perms.ctypes.data, out["losses"].ctypes.data, out["theta"].ctypes.data,
                     out["obs_mean"].ctypes.data, out["obs_var"].ctypes.data, out["obs_count"].ctypes.data,
                     out["ret_mean"].ctypes.data, out["ret_var"].ctypes.data, out["ret_count"].ctypes.data, None)
    r = HostResult()
    if lib.ppo_host_learn_explicit(C.byref(a), C.byref(x), C.byref(r)) != 0:
        raise RuntimeError(r.error.decode())
    return out


def learn_curve(n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma=0.99, lam=0.95, seed=0, reference_loop=False, device=-1,
                obs_dim=18, act_dim=18, discrete=False, cliprange_vf=-1.0, discrete_kernels="generic", compute_dtype=0, nvec=None, masked=False, n_playback=0,
                host_step_fused=False, target_kl=0.0, rollout_resident=False, binary=False):
    """PPO2::learn on TargetEnv x n_envs (a learnable task, host/env/env_mock.hpp) behind VecEnv + EnvNormalize with the library's own exploration noise and shuffles:
    returns the mean un-normalised reward of every update's rollout [n_updates], the per-update mean losses and the final weights.
    discrete=True: DiscreteTargetEnv (act_dim categories) and a categorical handle; discrete_kernels="narrow": that handle is created with
    PPO_ACT_SHAPE_KERNELS (PPO2::action_dist_for), "pair": with PPO_ACT_PAIR_KERNELS (hidden [256, 256]: train8_kernel<cat[,mask]> +
    weight_grad_assemble_kernel), "generic" (the default): without either.
    compute_dtype=1 (PPO_BF16; default 0): the handle runs the bf16 path; a discrete Env's handle is then created with PPO_ACT_BF16_HEAD, a multi-discrete Env's (nvec) with
    PPO_ACT_BF16_MULTI_HEAD (bf16_sample_kernel / bf16_loss_kernel<mcat[,mask]>, sum(nvec) <= 128).
    nvec=[n_0, ..]: MultiDiscreteTargetEnv with these components (act_dim is ignored: their sum) and a multi-categorical handle (PPO2::create_handle ->
    ppo_create_multi_ex; discrete_kernels="narrow": with PPO_ACT_SHAPE_KERNELS, the narrow <mcat> kernels where the shape qualifies; "pair": with
    PPO_ACT_PAIR_KERNELS, train8_kernel<mcat[,mask]> + weight_grad_assemble_kernel where hidden is [256, 256] and sum(nvec) <= 64), through ppo_host_learn_multi; masked=True: the environments also forbid about half of every component's categories per step (IActionMask)
    and the result carries "forbidden_received"; n_playback: that many PPO2::eval steps afterwards, "playback_actions" [n_playback, K] and "playback_legal".
    "kernel_counts": the handle's ppo_kernel_counts after the run.
    host_step_fused=True: ppo_set_host_step_fused(h, 1) on the created handle (ppo_host_args::host_step_fused): with discrete_kernels="narrow" and at most 32
    environments the act side runs narrow_host_step_kernel<cat|mcat[,mask]>, one launch per env step; nothing changes anywhere else.
    rollout_resident=True: ppo_set_rollout_resident(h, 1) on the created handle (through the process-wide default ppo_host_set_rollout_resident, cleared again when
    the call returns): with discrete_kernels="narrow" and at most 64 environments the rollout is served by the resident kernel's discrete forms
    (narrow_rollout_kernel<cat|mcat[,mask]>, one launch per rollout); nothing changes anywhere else.
    binary=True: MultiBinaryTargetEnv (act_dim bits, the IMultiBinary mixin) and a multi-binary handle (PPO2::create_handle -> ppo_create_ex with
    PPO_ACT_MULTI_BINARY), through ppo_host_learn_binary; discrete_kernels="binary_narrow" creates it with PPO_ACT_BINARY_SHAPE_KERNELS (narrow_step_kernel<mbin> /
    narrow_train_kernel<mbin> where the shape qualifies), "binary_pair" with PPO_ACT_BINARY_PAIR_KERNELS (train8_kernel<mbin> + weight_grad_assemble_kernel at hidden
    [256, 256]), the other words ask for the flags of a discrete Env's handle, which this head accepts and ignores; "kernel_counts" then holds every variant of the
    build (ppo_kernel_variant_name / ppo_kernel_count: a dict that grows between versions).  The head
    has no fused host step, no resident rollout, no masks and no bf16 path: host_step_fused, rollout_resident, masked, nvec, discrete and target_kl are refused with it.
    target_kl (default 0 = off): PPO2::set_target_kl, target-KL early stopping (include/ppo_hip.h, ppo_set_target_kl); "applied" [n_updates, 2] then holds the Adam
    steps applied / train steps of every update (ppo_host_explicit::target_kl / applied_out; not through the nvec form)."""
    lib = load_host_library()
    if binary:
        if host_step_fused or rollout_resident or masked or discrete or nvec is not None or target_kl or n_playback:
            raise ValueError("binary=True goes with none of host_step_fused, rollout_resident, masked, discrete, nvec, target_kl, n_playback")
        return _learn_binary(lib, n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma, lam, seed, reference_loop, device, obs_dim, act_dim,
                             cliprange_vf, discrete_kernels, compute_dtype)
    lib.ppo_host_set_rollout_resident(int(bool(rollout_resident)))
    try:
        return _learn_curve(lib, n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma, lam, seed, reference_loop, device, obs_dim, act_dim,
                            discrete, cliprange_vf, discrete_kernels, compute_dtype, nvec, masked, n_playback, host_step_fused, target_kl)
    finally:
        lib.ppo_host_set_rollout_resident(0)


def _learn_binary(lib, n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma, lam, seed, reference_loop, device, obs_dim, act_dim,
                  cliprange_vf, discrete_kernels, compute_dtype):
    import numpy as np
    a = HostArgs()
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.device, a.max_workers, a.reference_loop = device, 0, int(reference_loop)
    a.norm_obs, a.norm_reward, a.seed = 1, 1, seed
    a.obs_dim, a.act_dim, a.cliprange_vf, a.compute_dtype = obs_dim, act_dim, cliprange_vf, int(compute_dtype)
    a.discrete_kernels = _discrete_kernels(discrete_kernels)
    out = {"reward_curve": np.zeros(n_updates, np.float32), "losses": np.zeros((n_updates, 5), np.float32)}
    names = ((C.c_char * 32) * 64)(); cnt = (C.c_longlong * 64)(); ncnt = C.c_int(0)
    r = HostResult()
    fp = C.POINTER(C.c_float)
    if lib.ppo_host_learn_binary(C.byref(a), out["reward_curve"].ctypes.data_as(fp), out["losses"].ctypes.data_as(fp), names, cnt, C.byref(ncnt), C.byref(r)) != 0:
        raise RuntimeError(r.error.decode())
    out["kernel_counts"] = {names[i].value.decode(): int(cnt[i]) for i in range(ncnt.value)}
    return out


def _learn_curve(lib, n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma, lam, seed, reference_loop, device, obs_dim, act_dim,
                 discrete, cliprange_vf, discrete_kernels, compute_dtype, nvec, masked, n_playback, host_step_fused, target_kl):
    import numpy as np
    a = HostArgs()
    if nvec is not None:
        nvec = [int(x) for x in nvec]
        a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
        for i, h in enumerate(hidden):
            a.hidden[i] = h
        a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
        a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
        a.device, a.max_workers, a.reference_loop = device, 0, int(reference_loop)
        a.norm_obs, a.norm_reward, a.seed = 1, 1, seed
        a.obs_dim, a.act_dim, a.cliprange_vf, a.compute_dtype = obs_dim, sum(nvec), cliprange_vf, int(compute_dtype)
        a.n_components, a.multi_masked = len(nvec), int(bool(masked))
        a.discrete_kernels = _discrete_kernels(discrete_kernels)
        a.host_step_fused = int(bool(host_step_fused))
        if target_kl:
            raise ValueError("target_kl is not carried through the nvec form")
        for i, x in enumerate(nvec):
            a.nvec[i] = x
        out = {"reward_curve": np.zeros(n_updates, np.float32), "playback_actions": np.zeros((n_playback, len(nvec)), np.float32),
               "playback_legal": np.zeros(n_playback, np.float32)}
        names = ((C.c_char * 32) * 64)(); cnt = (C.c_longlong * 64)(); ncnt = C.c_int(0)
        forbidden = C.c_longlong(-1)
        r = HostResult()
        fp = C.POINTER(C.c_float)
        if lib.ppo_host_learn_multi(C.byref(a), out["reward_curve"].ctypes.data_as(fp), C.byref(forbidden), int(n_playback), out["playback_actions"].ctypes.data_as(fp),
                                    out["playback_legal"].ctypes.data_as(fp), names, cnt, C.byref(ncnt), C.byref(r)) != 0:
            raise RuntimeError(r.error.decode())
        out["forbidden_received"] = int(forbidden.value)
        out["kernel_counts"] = {names[i].value.decode(): int(cnt[i]) for i in range(ncnt.value)}
        return out
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.seeded_env, a.device, a.max_workers, a.reference_loop = 3 if discrete else 2, device, 0, int(reference_loop)
    a.norm_obs, a.norm_reward, a.seed = 1, 1, seed
    a.obs_dim, a.act_dim = obs_dim, act_dim
    a.cliprange_vf = cliprange_vf
    a.discrete_kernels = _discrete_kernels(discrete_kernels)
    a.compute_dtype = int(compute_dtype)
    a.host_step_fused = int(bool(host_step_fused))
    out = {"losses": np.zeros((n_updates, 5), np.float32), "reward_curve": np.zeros(n_updates, np.float32), "applied": np.zeros((n_updates, 2), np.int32)}
    names = ((C.c_char * 32) * 64)(); cnt = (C.c_longlong * 64)(); ncnt = C.c_int(0)
    x = HostExplicit(None, None, None, out["losses"].ctypes.data, None, None, None, None, None, None, None, out["reward_curve"].ctypes.data,
                     C.addressof(names), C.addressof(cnt), C.addressof(ncnt), out["applied"].ctypes.data, float(target_kl))
    r = HostResult()
    if lib.ppo_host_learn_explicit(C.byref(a), C.byref(x), C.byref(r)) != 0:
        raise RuntimeError(r.error.decode())
    out["kernel_counts"] = {names[i].value.decode(): int(cnt[i]) for i in range(ncnt.value)}
    out["env_steps_per_s"] = r.env_steps_per_s
    return out


def learn_time_limit(n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, time_limit, probe_raw, bootstrap_truncated=True, gamma=0.99,
                     lam=0.95, seed=0, norm_obs=True, norm_reward=False, device=-1, obs_dim=18, act_dim=18, cliprange_vf=-1.0):
    """PPO2::learn on n_envs x TimeLimit(UnitRewardEnv, time_limit) (reward 1 per step, episodes end by the time limit only) behind VecEnv + EnvNormalize, with the
    library's own exploration noise and shuffles (ppo_host_learn_time_limit).  bootstrap_truncated = PPO2::bootstrap_truncated.  Returns the critic on
    probe_raw [n, obs_dim] (n a multiple of n_envs; scaled with the final observation statistics) and the per-update mean losses."""
    import numpy as np
    lib = load_host_library()
    a = HostArgs()
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.seeded_env, a.device, a.max_workers, a.reference_loop = 0, device, 0, 0
    a.norm_obs, a.norm_reward, a.seed = int(norm_obs), int(norm_reward), seed
    a.obs_dim, a.act_dim = obs_dim, act_dim
    a.cliprange_vf = cliprange_vf
    probe = np.ascontiguousarray(probe_raw, np.float32)
    assert probe.ndim == 2 and probe.shape[1] == obs_dim and probe.shape[0] % n_envs == 0, probe.shape
    out = {"probe_values": np.zeros(probe.shape[0], np.float32), "losses": np.zeros((n_updates, 5), np.float32)}
    r = HostResult()
    fp = C.POINTER(C.c_float)
    if lib.ppo_host_learn_time_limit(C.byref(a), int(time_limit), int(bool(bootstrap_truncated)), probe.ctypes.data_as(fp), probe.shape[0],
                                     out["probe_values"].ctypes.data_as(fp), out["losses"].ctypes.data_as(fp), C.byref(r)) != 0:
        raise RuntimeError(r.error.decode())
    return out


def learn_masked(n_envs, n_steps, hidden, n_updates, nminibatches, noptepochs, lr, cliprange, gamma=0.99, lam=0.95, seed=0, reference_loop=False, device=-1,
                 obs_dim=18, act_dim=18, n_playback=0, cliprange_vf=-1.0, discrete_kernels="generic", compute_dtype=0, host_step_fused=False, rollout_resident=False):
    """PPO2::learn on MaskedTargetEnv x n_envs (host/env/env_mock.hpp: DiscreteTargetEnv's task with about half of the categories forbidden at every step) behind
    VecEnv + EnvNormalize, with the library's own exploration noise and shuffles (ppo_host_learn_masked).  PPO2 finds the IActionMask mixin and masks by itself.
    Returns the mean un-normalised reward of every update's rollout [n_updates], the count of forbidden actions the environments received over the whole run, and
    n_playback deterministic playback actions with their legality.  discrete_kernels, compute_dtype, host_step_fused, rollout_resident: as in learn_curve.
    "kernel_counts": the handle's ppo_kernel_counts after the run."""
    import numpy as np
    lib = load_host_library()
    a = HostArgs()
    a.n_envs, a.n_steps, a.n_hidden = n_envs, n_steps, len(hidden)
    for i, h in enumerate(hidden):
        a.hidden[i] = h
    a.nminibatches, a.noptepochs, a.n_updates = nminibatches, noptepochs, n_updates
    a.lr, a.cliprange, a.gamma, a.lam = lr, cliprange, gamma, lam
    a.seeded_env, a.device, a.max_workers, a.reference_loop = 0, device, 0, int(reference_loop)
    a.norm_obs, a.norm_reward, a.seed = 1, 1, seed
    a.obs_dim, a.act_dim = obs_dim, act_dim
    a.cliprange_vf = cliprange_vf
    a.discrete_kernels = _discrete_kernels(discrete_kernels)
    a.compute_dtype = int(compute_dtype)
    a.host_step_fused = int(bool(host_step_fused))
    out = {"reward_curve": np.zeros(n_updates, np.float32), "playback_actions": np.zeros(n_playback, np.float32), "playback_legal": np.zeros(n_playback, np.float32)}
    forbidden = C.c_longlong(-1)
    r = HostResult()
    fp = C.POINTER(C.c_float)
    lib.ppo_host_set_rollout_resident(int(bool(rollout_resident)))
    try:
        rc = lib.ppo_host_learn_masked(C.byref(a), out["reward_curve"].ctypes.data_as(fp), C.byref(forbidden), int(n_playback), out["playback_actions"].ctypes.data_as(fp),
                                       out["playback_legal"].ctypes.data_as(fp), C.byref(r))
    finally:
        lib.ppo_host_set_rollout_resident(0)
    if rc != 0:
        raise RuntimeError(r.error.decode())
    out["forbidden_received"] = int(forbidden.value)
    names = ((C.c_char * 32) * 64)(); cnt = (C.c_longlong * 64)()
    n = lib.ppo_host_last_kernel_counts(64, names, cnt)
    out["kernel_counts"] = {names[i].value.decode(): int(cnt[i]) for i in range(n)}
    return out


def value_clip_checkpoint(prefix, cliprange_vf):
    """PPO2::save of a policy built with cliprange_vf, PPO2::load into a fresh handle (ppo_host_value_clip_checkpoint): returns the fresh handle's
    value clipping as (mode, range), mode 0 / 1 / 2 = PPO_VCLIP_POLICY / RANGE / OFF"""
    lib = load_host_library()
    m, r = C.c_int32(), C.c_float()
    if lib.ppo_host_value_clip_checkpoint(prefix.encode(), C.c_float(cliprange_vf), C.byref(m), C.byref(r)) != 0:
        raise RuntimeError("ppo_host_value_clip_checkpoint failed (see stderr)")
    return m.value, r.value


def target_kl_checkpoint(prefix, target_kl, strip_key=False):
    """PPO2::save of a policy with set_target_kl(target_kl), PPO2::load into a fresh handle (ppo_host_target_kl_checkpoint): returns the fresh handle's
    target_kl.  strip_key: the "target_kl" key is removed from the side-car before the load (a checkpoint from before the setting)."""
    lib = load_host_library()
    x = C.c_float(-1.0)
    if lib.ppo_host_target_kl_checkpoint(prefix.encode(), C.c_float(target_kl), int(bool(strip_key)), C.byref(x)) != 0:
        raise RuntimeError("ppo_host_target_kl_checkpoint failed (see stderr)")
    return x.value


def multi_checkpoint(prefix, obs, nvec, other_nvec):
    """PPO2::save of a multi-categorical policy with components nvec, PPO2::load into a fresh handle with the same components, into one with other_nvec (another
    split of the same width) and into a plain categorical one (ppo_host_multi_checkpoint): returns (status, deterministic actions before [n, K], after);
    status 0 = identical tensors and both foreign loads refused"""
    import numpy as np
    lib = load_host_library()
    obs = np.ascontiguousarray(obs, np.float32)
    n, K = obs.shape[0], len(nvec)
    assert sum(nvec) == sum(other_nvec)
    acts = np.zeros((2, n, K), np.float32)
    nv, ov = (C.c_int * K)(*nvec), (C.c_int * len(other_nvec))(*other_nvec)
    rc = lib.ppo_host_multi_checkpoint(prefix.encode(), nv, ov, K, len(other_nvec), obs.ctypes.data_as(C.POINTER(C.c_float)), n, acts.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, acts[0], acts[1]


def discrete_checkpoint(prefix, obs):
    """PPO2::save of a categorical policy, PPO2::load into a fresh categorical handle and into a Gaussian one (ppo_host_discrete_checkpoint):
    returns (status, deterministic actions before, after); status 0 = identical tensors and the Gaussian load refused"""
    import numpy as np
    lib = load_host_library()
    obs = np.ascontiguousarray(obs, np.float32)
    n = obs.shape[0]
    acts = np.zeros((2, n), np.float32)
    rc = lib.ppo_host_discrete_checkpoint(prefix.encode(), obs.ctypes.data_as(C.POINTER(C.c_float)), n, acts.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, acts[0], acts[1]


def binary_checkpoint(prefix, obs, discrete_kernels="generic"):
    """PPO2::save of a multi-binary policy of 6 bits, PPO2::load into a fresh multi-binary handle, into a categorical one of the same width, and of a categorical
    policy's checkpoint (written under prefix + ".cat") into the multi-binary handle (ppo_host_binary_checkpoint_ex): returns (status, deterministic actions before
    [n, 6], after); status 0 = identical tensors and both foreign loads refused.  discrete_kernels="binary_narrow": both multi-binary handles are created with
    PPO_ACT_BINARY_SHAPE_KERNELS; "binary_pair": with PPO_ACT_BINARY_PAIR_KERNELS, every handle at hidden [256, 256]."""
    import numpy as np
    lib = load_host_library()
    obs = np.ascontiguousarray(obs, np.float32)
    n = obs.shape[0]
    acts = np.zeros((2, n, 6), np.float32)
    rc = lib.ppo_host_binary_checkpoint_ex(prefix.encode(), obs.ctypes.data_as(C.POINTER(C.c_float)), n, acts.ctypes.data_as(C.POINTER(C.c_float)),
                                           _discrete_kernels(discrete_kernels))
    return rc, acts[0], acts[1]


def policy_query(g, obs, actions, mask=None):
    """The host layer's policy queries on a capi.PPOHip handle `g` (ppo_host_policy_query): MlpPolicy::evaluate_actions, MlpPolicy::proba_step and
    PPO2::action_probability with the actions, plain and with logp.  Returns {"values", "neglogps", "entropies", "prob", "logprob": (n,); "params": (n, W)}."""
    import numpy as np
    lib = load_host_library()
    obs = np.ascontiguousarray(obs, np.float32); n = obs.shape[0]
    actions = np.ascontiguousarray(actions, np.float32).reshape(n, g.action_width)
    mk = np.ascontiguousarray(mask, np.float32).reshape(n, g.A) if mask is not None else None
    out = {k: np.zeros(n, np.float32) for k in ("values", "neglogps", "entropies", "prob", "logprob")}
    out["params"] = np.zeros((n, g.distribution_width), np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    if lib.ppo_host_policy_query(g.h, fp(obs), obs.shape[1], fp(actions), fp(mk) if mk is not None else None, g.A, n, fp(out["values"]), fp(out["neglogps"]),
                                 fp(out["entropies"]), fp(out["params"]), fp(out["prob"]), fp(out["logprob"])) != 0:
        raise RuntimeError("ppo_host_policy_query failed (message on stderr)")
    return out
