"""ctypes binding of libppo_hip.so (include/ppo_hip.h).  Thin: every method is one C-ABI call."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = None
MAX_LAYERS = 8


class PPOHipError(RuntimeError):
    pass


class PPOConfig(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * MAX_LAYERS), ("ent_coef", C.c_float), ("vf_coef", C.c_float),
                ("max_grad_norm", C.c_float), ("adam_beta1", C.c_float), ("adam_beta2", C.c_float),
                ("adam_eps", C.c_float), ("device", C.c_int32), ("max_rows", C.c_int32), ("compute_dtype", C.c_int32)]


def load_library(build=True):
    """Loads ppo_cpp_amd/libppo_hip.so (building it in-tree when the sources are newer)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(_PKG, "libppo_hip.so")
    alt = os.environ.get("PPO_HIP_LIBRARY")                  # a diagnostic build (tools/stamps*.py: -DPPO_STAMPS) kept OUTSIDE the package directory
    if alt:
        so = alt
    elif build and os.path.exists("/opt/rocm/bin/hipcc"):
        from . import build as _b
        so = _b.build_hip()
    if not os.path.exists(so):
        raise PPOHipError("libppo_hip.so is missing (%s): run `python -m ppo_cpp_amd.build`; there is no CPU fallback" % so)
    lib = C.CDLL(so)
    lib.ppo_last_error.restype = C.c_char_p
    lib.ppo_last_error.argtypes = [C.c_void_p]
    lib.ppo_destroy.argtypes = [C.c_void_p]
    lib.ppo_destroy.restype = None
    lib.ppo_kernel_count.restype = C.c_int64
    lib.ppo_kernel_count.argtypes = [C.c_void_p, C.c_char_p]
    lib.ppo_kernel_variant_name.restype = C.c_char_p
    lib.ppo_kernel_variant_name.argtypes = [C.c_int32]
    _LIB = lib
    return lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


ACTION_DISTS = {"gaussian": 0, "categorical": 1, "multi_categorical": 2, "multi_binary": 3}   # PPO_ACT_GAUSSIAN / PPO_ACT_CATEGORICAL / PPO_ACT_MULTI_CATEGORICAL / PPO_ACT_MULTI_BINARY
MAX_COMPONENTS = 16                                     # PPO_MAX_COMPONENTS
ACT_SHAPE_KERNELS = 0x100                               # PPO_ACT_SHAPE_KERNELS, OR-ed into ppo_create_ex's action_dist
ACT_BF16_HEAD = 0x200                                   # PPO_ACT_BF16_HEAD, likewise
ACT_PAIR_KERNELS = 0x400                                # PPO_ACT_PAIR_KERNELS, likewise
ACT_BF16_MULTI_HEAD = 0x1000                            # PPO_ACT_BF16_MULTI_HEAD, a flag of ppo_create_multi_ex only
ACT_BINARY_SHAPE_KERNELS = 0x2000                       # PPO_ACT_BINARY_SHAPE_KERNELS, a flag of ppo_create_ex beside PPO_ACT_MULTI_BINARY only
ACT_BINARY_PAIR_KERNELS = 0x4000                        # PPO_ACT_BINARY_PAIR_KERNELS, likewise
VALUE_CLIP_MODES = {"policy": 0, "range": 1, "off": 2}  # PPO_VCLIP_POLICY / PPO_VCLIP_RANGE / PPO_VCLIP_OFF


class PPOHip:
    """One handle = one GPU + stream; mirrors the TF session state of the reference (weights, Adam slots, beta
    powers) plus the device-resident rollout and normaliser.

    action_dist="categorical": act_dim is the number of categories; actions are (n,) float category indices
    (step / act_deterministic / rollout_act return them, train_step takes them, rollout_get("actions") is [T, E]);
    explicit noise keeps the Gaussian's shape and holds the uniforms of the Gumbel-argmax draw.
    shape_kernels=True (PPO_ACT_SHAPE_KERNELS; default False): a categorical handle whose shape qualifies (every hidden width <= 64, ...)
    runs the narrow LDS-resident kernels instead of the generic ones; any other shape, and a Gaussian handle, are not affected.
    bf16_head=True (PPO_ACT_BF16_HEAD; default False): with action_dist="categorical" and compute_dtype=1 (PPO_BF16) the handle runs the bf16
    matrix-core path with a categorical head (at most 128 categories; masks included; no data parallel).  Without it that combination is
    refused; on a compute_dtype=0 or Gaussian handle it changes nothing.
    pair_kernels=True (PPO_ACT_PAIR_KERNELS; default False): a categorical compute_dtype=0 handle with hidden [256, 256] and at most 64 observations /
    categories trains with train8_kernel<cat[,mask]> + weight_grad_assemble_kernel instead of the generic kernels (no data parallel); any other
    shape, a Gaussian handle and a compute_dtype=1 handle are not affected.

    action_dist="multi_categorical", nvec=[n_0, .., n_{K-1}] (ppo_create_multi): K independent categorical components over sum(nvec) logits;
    act_dim may be None or must equal sum(nvec).  Actions are (n, K) float arrays, column k the index within component k; noise and masks keep
    their (n, A) shape with A = sum(nvec).  `.nvec` reads the widths back from the handle (ppo_action_nvec).
    shape_kernels=True with it (ppo_create_multi_ex with PPO_ACT_SHAPE_KERNELS): the narrow LDS-resident kernels (narrow_step_kernel<mcat[,mask]>,
    narrow_train_kernel<mcat[,mask]>) where the shape qualifies as a categorical handle's would (hidden widths <= 64, sum(nvec) <= 64); any other
    shape runs the generic <mcat> kernels.  No data parallel on a handle the flag took effect on.
    pair_kernels=True with it (ppo_create_multi_ex with PPO_ACT_PAIR_KERNELS): hidden [256, 256] with at most 64 observations and sum(nvec) <= 64 trains with
    train8_kernel<mcat[,mask]> + weight_grad_assemble_kernel instead of train_fwd_bwd_kernel<mcat[,mask]> and its two followers (the act side is
    unchanged; no data parallel on a handle the flag took effect on); any other shape runs the generic <mcat> kernels.  shape_kernels and pair_kernels
    may be given together: their shape rules never both hold, each flag acts where its own rule holds.
    bf16_head=True with it and compute_dtype=1 (ppo_create_multi_ex with PPO_ACT_BF16_MULTI_HEAD): the bf16 matrix-core path with the multi-categorical
    head (bf16_sample_kernel / bf16_loss_kernel<mcat[,mask]>; sum(nvec) <= 128; masks included; no data parallel), e.g.
    PPOHip(O, None, hidden, action_dist="multi_categorical", nvec=[..], compute_dtype=1, bf16_head=True).  Without it that combination is refused; on a
    compute_dtype=0 handle bf16_head changes nothing (no flag is passed).

    action_dist="multi_binary" (PPO_ACT_MULTI_BINARY; stable-baselines' Bernoulli distribution over a MultiBinary space -- "bernoulli" is no action_dist here):
    act_dim independent on / off decisions per step.  Actions are (n, act_dim) float arrays of exactly 0 or 1 (train_step and rollout_set("actions") refuse anything
    else, naming row and column); explicit noise is (n, act_dim) uniforms, bit j is 1 where u_j < sigmoid(logit_j); act_deterministic gives logit_j > 0.  The tensor
    list is a categorical handle's (no pi/logstd), `.nvec` is [].  compute_dtype=0 only; the handle runs policy_step_kernel<mbin> / train_fwd_bwd_kernel<mbin> on any
    hidden widths, shape_kernels / pair_kernels / bf16_head are accepted and change nothing, and mask= raises the library's error.
    binary_shape_kernels=True with it (PPO_ACT_BINARY_SHAPE_KERNELS; default False; a ValueError with any other action_dist): a handle whose shape qualifies
    (every hidden width <= 64, at most 64 observations and bits, ...) runs narrow_step_kernel<mbin> / narrow_train_kernel<mbin> -- same arithmetic, the same draws for
    the same seed, no data parallel; set_host_step_fused / set_rollout_resident change nothing on it; any other shape runs the generic <mbin> kernels.  The two names
    are rows of kernel_counts(all_rows=True) only.  The attribute binary_shape_kernels keeps what was asked for.
    binary_pair_kernels=True with it (PPO_ACT_BINARY_PAIR_KERNELS; default False; a ValueError with any other action_dist): a handle of hidden [256, 256] with at
    most 64 observations and bits trains with train8_kernel<mbin> + weight_grad_assemble_kernel -- the act side stays policy_step_kernel<mbin> (same bits), no data
    parallel; any other shape runs the generic <mbin> kernels.  "train8_kernel<mbin>" is a name of kernel_count() / kernel_variants() only.  The attribute
    binary_pair_kernels keeps what was asked for.

    Action masks (categorical and multi-categorical; include/ppo_hip.h): step / act_deterministic / train_step take mask=(n, A), non-zero = allowed;
    set_action_masking(True) makes the rollout carry masks (rollout_act(t, mask=(E, A)), rollout_get / rollout_set("masks"))
    and update() train under them."""

    FIELDS = {"obs": 0, "actions": 1, "values": 2, "neglogp": 3, "dones": 4, "rewards": 5, "returns": 6}
    MASK_FIELDS = {"masks": 8}                  # [T, E, A]; a masking handle only (set_action_masking)
    OUTPUT_FIELDS = {"terminal_values": 7}      # rollout_get only: what the last rollout_finish computed beside the rollout itself (an upload is refused)

    def __init__(self, obs_dim, act_dim, hidden, device=-1, action_dist="gaussian", shape_kernels=False, bf16_head=False, nvec=None, pair_kernels=False, binary_shape_kernels=False,
                 binary_pair_kernels=False, **overrides):
        multi = action_dist == "multi_categorical"
        if binary_shape_kernels and action_dist != "multi_binary":
            raise ValueError("binary_shape_kernels belongs to action_dist='multi_binary', not %r" % (action_dist,))
        if binary_pair_kernels and action_dist != "multi_binary":
            raise ValueError("binary_pair_kernels belongs to action_dist='multi_binary', not %r" % (action_dist,))
        if nvec is not None and not multi:
            raise ValueError("nvec belongs to action_dist='multi_categorical', not %r" % (action_dist,))
        if multi:
            if nvec is None:
                raise ValueError("action_dist='multi_categorical' needs nvec")
            nvec = [int(x) for x in nvec]
            if act_dim is None:
                act_dim = sum(nvec)
            elif act_dim != sum(nvec):
                raise ValueError("act_dim %r is not sum(nvec) = %d" % (act_dim, sum(nvec)))
        self.lib = load_library()
        cfg = PPOConfig()
        hid = (C.c_int32 * len(hidden))(*hidden)
        self.lib.ppo_config_default(C.byref(cfg), obs_dim, act_dim, len(hidden), hid)
        cfg.device = device
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.O, self.A, self.hidden = obs_dim, act_dim, list(hidden)
        if action_dist not in ACTION_DISTS:
            raise ValueError("action_dist must be one of %s, not %r" % (sorted(ACTION_DISTS), action_dist))
        self.action_dist = action_dist
        self.shape_kernels = bool(shape_kernels)
        self.bf16_head = bool(bf16_head)
        self.pair_kernels = bool(pair_kernels)
        self.binary_shape_kernels = bool(binary_shape_kernels)
        self.binary_pair_kernels = bool(binary_pair_kernels)
        self._act_shape = (act_dim,) if action_dist in ("gaussian", "multi_binary") else (len(nvec),) if multi else ()      # per row
        h = C.c_void_p()
        if multi:
            nv = (C.c_int32 * max(len(nvec), 1))(*nvec)
            flags = (ACT_SHAPE_KERNELS if shape_kernels else 0) | (ACT_PAIR_KERNELS if pair_kernels else 0)
            if bf16_head and cfg.compute_dtype == 1:
                flags |= ACT_BF16_MULTI_HEAD
            if (self.lib.ppo_create_multi_ex(C.byref(cfg), nv, len(nvec), flags, C.byref(h)) if flags
                    else self.lib.ppo_create_multi(C.byref(cfg), nv, len(nvec), C.byref(h))) != 0:
                raise PPOHipError(self.lib.ppo_last_error(None).decode())
        elif self.lib.ppo_create_ex(C.byref(cfg), ACTION_DISTS[action_dist] | (ACT_SHAPE_KERNELS if shape_kernels else 0) | (ACT_BF16_HEAD if bf16_head else 0)
                                    | (ACT_PAIR_KERNELS if pair_kernels else 0) | (ACT_BINARY_SHAPE_KERNELS if binary_shape_kernels else 0)
                                    | (ACT_BINARY_PAIR_KERNELS if binary_pair_kernels else 0), C.byref(h)) != 0:
            raise PPOHipError(self.lib.ppo_last_error(None).decode())
        self.h = h
        self.P = self.lib.ppo_num_params(self.h)
        self.tensors = []
        for i in range(self.lib.ppo_num_tensors(self.h)):
            name = C.create_string_buffer(32)
            r, c = C.c_int32(), C.c_int32()
            self._ck(self.lib.ppo_tensor_info(self.h, i, name, C.byref(r), C.byref(c)))
            self.tensors.append((name.value.decode(), (r.value, c.value) if c.value else (r.value,)))
        self.E = self.T = 0
        self.world, self._global_shuffle = 1, False

    @property
    def nvec(self):
        """component widths as the handle reports them (ppo_action_nvec): [] Gaussian and multi-binary, [A] categorical, the K widths multi-categorical"""
        out = (C.c_int32 * MAX_COMPONENTS)()
        k = self.lib.ppo_action_nvec(self.h, MAX_COMPONENTS, out)
        return [int(out[i]) for i in range(max(k, 0))]

    @property
    def action_width(self):
        return int(self.lib.ppo_action_width(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ppo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise PPOHipError(self.lib.ppo_last_error(self.h).decode())

    # ---- variables --------------------------------------------------------------------------------
    def get_flat(self, which=0):
        out = np.empty(self.P, np.float32)
        self._ck(self.lib.ppo_get_flat(self.h, which, _fp(out), C.c_int64(self.P)))
        return out

    def set_flat(self, arr, which=0):
        a = _f32(arr, (self.P,))
        self._ck(self.lib.ppo_set_flat(self.h, which, _fp(a), C.c_int64(self.P)))

    def set_tensors(self, named):
        for i, (name, shape) in enumerate(self.tensors):
            a = _f32(named[name]).reshape(-1)
            self._ck(self.lib.ppo_set_tensor(self.h, 0, i, _fp(a), C.c_int64(a.size)))

    def get_tensor(self, name, which=0):
        for i, (n, shape) in enumerate(self.tensors):
            if n == name:
                out = np.empty(int(np.prod(shape)), np.float32)
                self._ck(self.lib.ppo_get_tensor(self.h, which, i, _fp(out), C.c_int64(out.size)))
                return out.reshape(shape)
        raise KeyError(name)

    def init_orthogonal(self, seed=0):
        self._ck(self.lib.ppo_init_orthogonal(self.h, C.c_uint64(seed)))

    def seed(self, seed):
        self._ck(self.lib.ppo_seed(self.h, C.c_uint64(seed)))

    def beta_powers(self):
        pw = np.empty(2, np.float32)
        self._ck(self.lib.ppo_get_beta_powers(self.h, _fp(pw)))
        return pw

    def set_beta_powers(self, pw):
        a = _f32(pw, (2,))
        self._ck(self.lib.ppo_set_beta_powers(self.h, _fp(a)))

    # ---- act model --------------------------------------------------------------------------------
    def step(self, obs, noise=None, mask=None):
        obs = _f32(obs); n = obs.shape[0]
        a = np.empty((n,) + self._act_shape, np.float32); v = np.empty(n, np.float32); nlp = np.empty(n, np.float32)
        nz = _f32(noise, (n, self.A)) if noise is not None else None
        if mask is not None:
            mk = _f32(mask, (n, self.A))
            self._ck(self.lib.ppo_step_masked(self.h, _fp(obs), n, _fp(nz) if nz is not None else None, _fp(mk), _fp(a), _fp(v), _fp(nlp)))
            return a, v, nlp
        self._ck(self.lib.ppo_step(self.h, _fp(obs), n, _fp(nz) if nz is not None else None, _fp(a), _fp(v), _fp(nlp)))
        return a, v, nlp

    def value(self, obs):
        obs = _f32(obs); n = obs.shape[0]
        v = np.empty(n, np.float32)
        self._ck(self.lib.ppo_value(self.h, _fp(obs), n, _fp(v)))
        return v

    def act_deterministic(self, obs, mask=None):
        obs = _f32(obs); n = obs.shape[0]
        a = np.empty((n,) + self._act_shape, np.float32)
        if mask is not None:
            mk = _f32(mask, (n, self.A))
            self._ck(self.lib.ppo_act_deterministic_masked(self.h, _fp(obs), n, _fp(mk), _fp(a)))
            return a
        self._ck(self.lib.ppo_act_deterministic(self.h, _fp(obs), n, _fp(a)))
        return a

    # ---- querying the policy (include/ppo_hip.h; stateless: no RNG advance, no rollout / normaliser / Adam state touched) -------
    @property
    def distribution_width(self):
        """W, the columns of one action_probability row: Gaussian 2A (mu | std), categorical A, multi-categorical sum(nvec), multi-binary A"""
        return int(self.lib.ppo_distribution_width(self.h))

    def evaluate_actions(self, obs, actions, mask=None):
        """(value, neglogp, entropy), each (n,): the current policy's value, the neglogp of the GIVEN actions and the rows' entropy (stable-baselines 3
        evaluate_actions).  actions as train_step takes them, mask as step takes it."""
        obs = _f32(obs); n = obs.shape[0]
        act = _f32(actions, (n,) + self._act_shape)
        mk = _f32(mask, (n, self.A)) if mask is not None else None
        v = np.empty(n, np.float32); nlp = np.empty(n, np.float32); ent = np.empty(n, np.float32)
        self._ck(self.lib.ppo_evaluate_actions(self.h, _fp(obs), _fp(act), n, _fp(mk) if mk is not None else None, _fp(v), _fp(nlp), _fp(ent)))
        return v, nlp, ent

    def action_probability(self, obs, mask=None):
        """(n, W) distribution parameters (stable-baselines 2 proba_step): Gaussian mu | std, categorical and multi-categorical the probabilities of every category
        (exactly 0 for a forbidden one), multi-binary P(bit = 1)."""
        obs = _f32(obs); n = obs.shape[0]
        mk = _f32(mask, (n, self.A)) if mask is not None else None
        out = np.empty((n, self.distribution_width), np.float32)
        self._ck(self.lib.ppo_action_probability(self.h, _fp(obs), n, _fp(mk) if mk is not None else None, _fp(out), C.c_int64(out.size)))
        return out

    def rollout_evaluate(self):
        """(value, neglogp, entropy), each (T, E): evaluate_actions over the finished device-resident rollout (its obs, actions and, on a masking handle, masks)
        under the current weights, without staging anything from the host"""
        outs = [np.empty((self.T, self.E), np.float32) for _ in range(3)]
        self._ck(self.lib.ppo_rollout_evaluate(self.h, *[_fp(x) for x in outs]))
        return tuple(outs)

    # ---- train ------------------------------------------------------------------------------------
    def train_step(self, lr, cliprange, obs, actions, advs, returns, old_nlp, old_v, mask=None):
        arrs = [_f32(x) for x in (obs, actions, advs, returns, old_nlp, old_v)]
        n = arrs[0].shape[0]
        if self.action_dist != "gaussian":
            arrs[1] = _f32(arrs[1], (n,) + self._act_shape)
        losses = np.empty(5, np.float32)
        if mask is not None:
            arrs.insert(2, _f32(mask, (n, self.A)))
            self._ck(self.lib.ppo_train_step_masked(self.h, C.c_float(lr), C.c_float(cliprange), *[_fp(x) for x in arrs], n, _fp(losses)))
            return losses
        self._ck(self.lib.ppo_train_step(self.h, C.c_float(lr), C.c_float(cliprange), *[_fp(x) for x in arrs], n, _fp(losses)))
        return losses

    def set_value_clip(self, mode, range=0.0):
        """Value-function clipping from the next train_step / update on: "policy" (0, the default: clip with cliprange), "range" (1: clip with
        `range`, finite and >= 0) or "off" (2: the unclipped (v - R)^2).  `range` is ignored outside "range"."""
        m = VALUE_CLIP_MODES.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(mode, str) and mode not in VALUE_CLIP_MODES:
            raise ValueError("mode must be one of %s or an int, not %r" % (sorted(VALUE_CLIP_MODES), mode))
        self._ck(self.lib.ppo_set_value_clip(self.h, C.c_int32(int(m)), C.c_float(range)))

    def get_value_clip(self):
        """(mode name, range): range is 0.0 outside "range" """
        m, r = C.c_int32(), C.c_float()
        self._ck(self.lib.ppo_get_value_clip(self.h, C.byref(m), C.byref(r)))
        return {v: k for k, v in VALUE_CLIP_MODES.items()}[m.value], r.value

    def set_target_kl(self, target_kl):
        """Target-KL early stopping from the next train_step / update on (include/ppo_hip.h, ppo_set_target_kl): a train step whose approxkl (losses[3], the
        project's half mean squared log-ratio) exceeds 1.5 * target_kl is not applied and ends the update.  0 = off (the default); a negative, NaN or infinite
        value, a PPO_BF16 handle and a handle with a communicator are errors that leave the previous setting in place."""
        self._ck(self.lib.ppo_set_target_kl(self.h, C.c_float(target_kl)))

    def target_kl(self):
        x = C.c_float()
        self._ck(self.lib.ppo_get_target_kl(self.h, C.byref(x)))
        return x.value

    def update_applied(self):
        """(Adam steps applied, train steps enqueued) of the last update() or train_step(); with target_kl off both are the number of train steps"""
        a, t = C.c_int32(), C.c_int32()
        self._ck(self.lib.ppo_update_applied(self.h, C.byref(a), C.byref(t)))
        return a.value, t.value

    def last_grad(self):
        g = np.empty(self.P, np.float32); norm = C.c_float()
        self._ck(self.lib.ppo_get_last_grad(self.h, _fp(g), C.c_int64(self.P), C.byref(norm)))
        return g, norm.value

    def adv_normalize(self, returns, values):
        r, v = _f32(returns), _f32(values)
        out = np.empty_like(r)
        self._ck(self.lib.ppo_adv_normalize(self.h, _fp(r), _fp(v), r.size, _fp(out)))
        return out

    def gae(self, rewards, values, dones, last_values, last_dones, gamma, lam, terminal_values=None):
        """terminal_values [T, E]: V(terminal observation) on the rows cut by a time limit, 0 elsewhere (ppo_gae_ex); None = every done is terminal (ppo_gae)"""
        rw, va, dn, lv, ld = [_f32(x) for x in (rewards, values, dones, last_values, last_dones)]
        T, E = rw.shape
        out = np.empty((T, E), np.float32)
        if terminal_values is None:
            self._ck(self.lib.ppo_gae(self.h, _fp(rw), _fp(va), _fp(dn), _fp(lv), _fp(ld), T, E, C.c_float(gamma), C.c_float(lam), _fp(out)))
        else:
            tv = _f32(terminal_values, (T, E))
            self._ck(self.lib.ppo_gae_ex(self.h, _fp(rw), _fp(va), _fp(dn), _fp(lv), _fp(ld), _fp(tv), T, E, C.c_float(gamma), C.c_float(lam), _fp(out)))
        return out

    # ---- normaliser -------------------------------------------------------------------------------
    def norm_init(self, n_envs, gamma=0.99, clip_obs=10.0, clip_rew=10.0, eps=1e-8):
        self._ck(self.lib.ppo_norm_init(self.h, n_envs, C.c_float(gamma), C.c_float(clip_obs), C.c_float(clip_rew), C.c_float(eps)))

    def norm_set_flags(self, norm_obs=True, norm_reward=True):
        self._ck(self.lib.ppo_norm_set_flags(self.h, int(norm_obs), int(norm_reward)))

    def norm_reset_returns(self):
        self._ck(self.lib.ppo_norm_reset_returns(self.h))

    def norm_obs(self, raw, training=True):
        x = _f32(raw); out = np.empty_like(x)
        self._ck(self.lib.ppo_norm_obs(self.h, _fp(x), x.shape[0], int(training), _fp(out)))
        return out

    def norm_reward(self, rew, dones, training=True):
        r, d = _f32(rew).reshape(-1), _f32(dones).reshape(-1); out = np.empty_like(r)
        self._ck(self.lib.ppo_norm_reward(self.h, _fp(r), _fp(d), r.size, int(training), _fp(out)))
        return out

    def norm_stats(self, which):
        dim = self.O if which == 0 else 1
        mean = np.empty(dim, np.float32); var = np.empty(dim, np.float32); cnt = C.c_double()
        self._ck(self.lib.ppo_norm_get_stats(self.h, which, _fp(mean), _fp(var), C.byref(cnt)))
        return mean, var, cnt.value

    def set_norm_stats(self, which, mean, var, count):
        m, v = _f32(mean).reshape(-1), _f32(var).reshape(-1)
        self._ck(self.lib.ppo_norm_set_stats(self.h, which, _fp(m), _fp(v), C.c_double(count)))

    # ---- rollout ----------------------------------------------------------------------------------
    def rollout_alloc(self, n_envs, n_steps):
        self._ck(self.lib.ppo_rollout_alloc(self.h, n_envs, n_steps))
        self.E, self.T = n_envs, n_steps

    def rollout_reset(self, raw_obs):
        x = _f32(raw_obs, (self.E, self.O))
        self._ck(self.lib.ppo_rollout_reset(self.h, _fp(x)))

    def set_action_masking(self, on=True):
        """Masks in the device-resident rollout and in update() (include/ppo_hip.h, ppo_set_action_masking).  Changing the setting drops an
        allocated rollout: call rollout_alloc again."""
        self._ck(self.lib.ppo_set_action_masking(self.h, int(bool(on))))

    def get_action_masking(self):
        return bool(self.lib.ppo_get_action_masking(self.h))

    def set_host_step_fused(self, on=True):
        """One launch per env step behind a host Env for a narrow categorical / multi-categorical handle (include/ppo_hip.h, ppo_set_host_step_fused): takes effect
        with shape_kernels on a qualifying shape, at most 32 environments, no communicator; any other handle accepts it and nothing changes (kernel_counts says
        which ran).  Call it before rollout_alloc: changing the setting drops an allocated rollout."""
        self._ck(self.lib.ppo_set_host_step_fused(self.h, int(bool(on))))

    @property
    def host_step_fused(self):
        """the setting, not whether it took effect"""
        return bool(self.lib.ppo_host_step_fused(self.h))

    def set_rollout_resident(self, on=True):
        """One launch per rollout for a narrow categorical / multi-categorical handle (include/ppo_hip.h, ppo_set_rollout_resident): collect_synthetic and, behind
        a host Env without explicit noise, rollout_act / rollout_observe are served by the resident kernel's discrete forms.  Takes effect with shape_kernels on a
        qualifying shape, at most 64 environments, no communicator; any other handle accepts it and nothing changes (kernel_counts says which ran).  Call it before
        rollout_alloc: changing the setting drops an allocated rollout."""
        self._ck(self.lib.ppo_set_rollout_resident(self.h, int(bool(on))))

    @property
    def rollout_resident(self):
        """the setting, not whether it took effect"""
        return bool(self.lib.ppo_rollout_resident(self.h))

    def rollout_act(self, t, noise=None, mask=None):
        out = np.empty((self.E,) + self._act_shape, np.float32)
        nz = _f32(noise, (self.E, self.A)) if noise is not None else None
        if mask is not None:
            mk = _f32(mask, (self.E, self.A))
            self._ck(self.lib.ppo_rollout_act_masked(self.h, t, _fp(nz) if nz is not None else None, _fp(mk), _fp(out)))
            return out
        self._ck(self.lib.ppo_rollout_act(self.h, t, _fp(nz) if nz is not None else None, _fp(out)))
        return out

    def rollout_observe(self, t, raw_obs, raw_rew, dones):
        o, r, d = _f32(raw_obs, (self.E, self.O)), _f32(raw_rew).reshape(-1), _f32(dones).reshape(-1)
        self._ck(self.lib.ppo_rollout_observe(self.h, t, _fp(o), _fp(r), _fp(d)))

    def rollout_mark_truncated(self, t, env_ids, terminal_raw_obs):
        """the dones of step t of `env_ids` were time-limit truncations; terminal_raw_obs [len(env_ids), O] = the raw observations those episodes ended on.
        Call it after rollout_observe(t, ..) and before the next rollout_act / rollout_finish (include/ppo_hip.h, ppo_rollout_mark_truncated)."""
        ids = np.ascontiguousarray(env_ids, np.int32).reshape(-1)
        obs = _f32(terminal_raw_obs).reshape(ids.size, self.O)
        self._ck(self.lib.ppo_rollout_mark_truncated(self.h, int(t), int(ids.size), ids.ctypes.data_as(C.POINTER(C.c_int32)), _fp(obs)))

    def rollout_finish(self, gamma, lam):
        self._ck(self.lib.ppo_rollout_finish(self.h, C.c_float(gamma), C.c_float(lam)))

    def collect_synthetic(self, seed, gamma, lam, noise=None, env0=0, step0=0, first=True):
        nz = _f32(noise, (self.T, self.E, self.A)) if noise is not None else None
        self._ck(self.lib.ppo_collect_synthetic(self.h, C.c_uint32(seed), env0, C.c_uint32(step0), int(first),
                                                _fp(nz) if nz is not None else None, C.c_float(gamma), C.c_float(lam)))

    def rollout_get(self, field):
        shape = {"obs": (self.T, self.E, self.O), "actions": (self.T, self.E) + self._act_shape, "masks": (self.T, self.E, self.A)}.get(field, (self.T, self.E))
        out = np.empty(shape, np.float32)
        idx = self.FIELDS[field] if field in self.FIELDS else self.MASK_FIELDS[field] if field in self.MASK_FIELDS else self.OUTPUT_FIELDS[field]
        self._ck(self.lib.ppo_rollout_download(self.h, idx, _fp(out), C.c_int64(out.size)))
        return out

    def rollout_set(self, field, arr):
        a = _f32(arr)
        idx = self.FIELDS[field] if field in self.FIELDS else self.MASK_FIELDS[field] if field in self.MASK_FIELDS else self.OUTPUT_FIELDS[field]
        self._ck(self.lib.ppo_rollout_upload(self.h, idx, _fp(a), C.c_int64(a.size)))

    def update(self, lr, cliprange, noptepochs, nminibatches, perms=None, seed=0, want_rows=True):
        rows = np.empty((noptepochs * nminibatches, 5), np.float32) if want_rows else None
        mean = np.empty(5, np.float32)
        pp = None
        if perms is not None:
            perms = np.ascontiguousarray(perms, np.int32)
            cols = self.E * self.T * (self.world if self._global_shuffle else 1)      # (B * world columns under ppo_dist_global_shuffle)
            assert perms.shape == (noptepochs, cols), (perms.shape, (noptepochs, cols))
            pp = perms.ctypes.data_as(C.POINTER(C.c_int32))
        self._ck(self.lib.ppo_update(self.h, C.c_float(lr), C.c_float(cliprange), noptepochs, nminibatches, pp, C.c_uint64(seed),
                                     _fp(rows) if rows is not None else None, _fp(mean)))
        return rows, mean

    # ---- dist / measurement -----------------------------------------------------------------------
    @staticmethod
    def dist_unique_id():
        lib = load_library()
        uid = C.create_string_buffer(128)
        if lib.ppo_dist_unique_id(uid) != 0:
            raise PPOHipError(lib.ppo_last_error(None).decode())
        return uid.raw

    def dist_init(self, world, rank, uid):
        assert len(uid) == 128
        self._ck(self.lib.ppo_dist_init(self.h, world, rank, C.create_string_buffer(uid, 128)))
        self.world = world

    def dist_info(self):
        """{comm_nranks (ncclCommCount), device (HIP ordinal), pci_bus_id, library (path of the collective library loaded)}"""
        n, d = C.c_int32(), C.c_int32()
        pci, lib = C.create_string_buffer(32), C.create_string_buffer(256)
        self._ck(self.lib.ppo_dist_info(self.h, C.byref(n), C.byref(d), pci, lib))
        return {"comm_nranks": n.value, "device": d.value, "pci_bus_id": pci.value.decode(), "library": lib.value.decode()}

    def dist_graph_collectives(self):
        return bool(self.lib.ppo_dist_graph_collectives(self.h))

    def dist_peer_export(self):
        """64-byte IPC handle of this rank's gather region (one-shot peer all-reduce); all-gather them and pass to dist_peer_attach"""
        buf = C.create_string_buffer(64)
        self._ck(self.lib.ppo_dist_peer_export(self.h, buf))
        return buf.raw

    def dist_peer_attach(self, handles):
        """handles: world x 64 bytes in rank order.  Collective.  Returns True when the peer path is now in use."""
        blob = b"".join(handles) if not isinstance(handles, (bytes, bytearray)) else bytes(handles)
        self._ck(self.lib.ppo_dist_peer_attach(self.h, C.create_string_buffer(blob, len(blob))))
        return self.dist_peer_active()

    def dist_peer_active(self):
        return bool(self.lib.ppo_dist_peer_active(self.h))

    def dist_global_shuffle(self, on=True):
        self._ck(self.lib.ppo_dist_global_shuffle(self.h, int(on)))
        self._global_shuffle = bool(on) and self.world > 1

    def dist_bucketed(self, on=True):
        """bf16 path under a communicator: gradient buckets on a second stream (True, the default) / one all-reduce (False) / 2: buckets also at world 1 (measurement)"""
        self._ck(self.lib.ppo_dist_bucketed(self.h, int(on)))

    def dist_peer_enable(self, on=True):
        self._ck(self.lib.ppo_dist_peer_enable(self.h, int(on)))

    def prof_enable(self, on=True):
        self._ck(self.lib.ppo_prof_enable(self.h, int(on)))

    def prof_read(self):
        names = ((C.c_char * 32) * 16)(); ms = (C.c_double * 16)(); cnt = (C.c_int64 * 16)()
        n = self.lib.ppo_prof_read(self.h, 16, names, ms, cnt)
        return {names[i].value.decode(): (ms[i], cnt[i]) for i in range(n)}

    def kernel_counts(self, all_rows=False):
        """{kernel variant: times enqueued since creation} -- which of the shape-selected kernels the calls so far took.  The default is ppo_kernel_counts' frozen
        60 rows; all_rows=True (ppo_kernel_counts_all) adds narrow_step_kernel<mbin> and narrow_train_kernel<mbin>: 62 rows, frozen as well.  Variants named
        after those are in kernel_variants() / kernel_count(name) only."""
        names = ((C.c_char * 32) * 64)(); cnt = (C.c_int64 * 64)()
        n = (self.lib.ppo_kernel_counts_all if all_rows else self.lib.ppo_kernel_counts)(self.h, 64, names, cnt)
        return {names[i].value.decode(): cnt[i] for i in range(n)}

    def kernel_count(self, name):
        """times the kernel variant `name` was enqueued since creation (ppo_kernel_count): any variant of this build, e.g. "train8_kernel<mbin>"; -1 where no
        variant has that name"""
        return int(self.lib.ppo_kernel_count(self.h, name.encode()))

    def kernel_variants(self):
        """{kernel variant: times enqueued since creation} over EVERY variant of this build (ppo_kernel_variant_name / ppo_kernel_count).  This dict GROWS between
        versions: look names up in it, never hold its length.  (kernel_counts() and kernel_counts(all_rows=True) are its first 60 / 62 entries, frozen.)"""
        out, i = {}, 0
        while True:
            name = self.lib.ppo_kernel_variant_name(i)
            if name is None:
                return out
            out[name.decode()] = int(self.lib.ppo_kernel_count(self.h, name))
            i += 1

    def debug_buffer(self, name):
        """a raw device buffer by name, padding included, as uint32 words (include/ppo_hip.h, ppo_debug_buffer); empty when this shape does not use it"""
        cnt = C.c_int64(0)
        self._ck(self.lib.ppo_debug_buffer(self.h, name.encode(), None, C.c_int64(0), C.byref(cnt)))
        out = np.empty(cnt.value, np.uint32)
        if cnt.value:
            self._ck(self.lib.ppo_debug_buffer(self.h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(cnt.value), C.byref(cnt)))
        return out

    def debug_graph_nodes(self):
        """{kernel, memset, memcpy, other: count} of the update's captured hipGraph, or None when the handle holds none (include/ppo_hip.h, ppo_debug_graph_nodes)"""
        c = (C.c_int32 * 4)()
        if self.lib.ppo_debug_graph_nodes(self.h, c) != 0:
            return None
        return dict(zip(("kernel", "memset", "memcpy", "other"), [int(x) for x in c]))

    def debug_raise_chain_error(self):
        self._ck(self.lib.ppo_debug_raise_chain_error(self.h))

    def debug_poison_lds(self, word=0x7FC0DEAD):
        """leave `word` (default: a NaN pattern) in every LDS word of every CU (include/ppo_hip.h, ppo_debug_poison_lds)"""
        self._ck(self.lib.ppo_debug_poison_lds(self.h, C.c_uint32(word)))

    def sync(self):
        self._ck(self.lib.ppo_sync(self.h))
