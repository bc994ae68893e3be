"""Host-side scheduler logic: mirrors the interface `AudioDiffusion.inference` touches on the
reference scheduler object (`set_timesteps`, `timesteps`, `order`, `init_noise_sigma`,
`scale_model_input`, `step(...).prev_sample`, `config`) -- reference:
mustango/diffusers/src/diffusers/schedulers/scheduling_ddpm.py:123-349 and scheduling_ddim.py:120-360.

The tensor math of `step` runs inside the engine's fused CFG+step kernel; this module only produces
the integer timestep schedule (bit-exact requirement) and the per-step fp32 coefficient table the
kernel consumes.  Tables are computed with torch fp32 CPU ops in the reference's own order
(`linspace(sqrt(b0), sqrt(b1), T)**2`, `cumprod`) so the scalars are bit-identical to the reference's.
"""
import copy
from types import SimpleNamespace

import numpy as np
import torch

#: stabilityai/stable-diffusion-2-1 `scheduler/scheduler_config.json` (tango.py:36 fetches it from the
#: hub; not in the tree).  The engine takes the config as data -- pass a different dict to override.
SD21_SCHEDULER_CONFIG = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                             beta_schedule="scaled_linear", prediction_type="v_prediction",
                             clip_sample=False, variance_type="fixed_small", clip_sample_range=1.0,
                             set_alpha_to_one=False, steps_offset=1)


class _StepOutput:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


class _AddNoise:
    """`add_noise` and the per-step table of its scalars, shared by every scheduler here: the fork's add_noise is one function in
    scheduling_ddpm.py:351-371, scheduling_ddim.py:361-381 and scheduling_dpmsolver_multistep.py:510-530"""

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(abar_t) * original_samples + sqrt(1 - abar_t) * noise per batch row, in the sample's dtype and device"""
        ac = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        timesteps = torch.as_tensor(timesteps).to(original_samples.device)
        sa = (ac[timesteps] ** 0.5).flatten()
        while len(sa.shape) < len(original_samples.shape):
            sa = sa.unsqueeze(-1)
        sb = ((1 - ac[timesteps]) ** 0.5).flatten()
        while len(sb.shape) < len(original_samples.shape):
            sb = sb.unsqueeze(-1)
        return sa * original_samples + sb * noise

    def blend_table(self, start=0) -> np.ndarray:
        """[N - start, 2] fp32: add_noise's scalars sqrt(abar_t), sqrt(1 - abar_t) at the set timesteps from index `start` on (the
        masked loop's blend, include/tango_engine.h tango_denoise_args_t.blend_coef; start > 0: a truncated loop, edit_plan())"""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() before blend_table()")
        start = self._check_start(start)
        t = torch.as_tensor(self.timesteps).to(torch.int64)[start:]
        ac = self.alphas_cumprod.to(torch.float32)
        return torch.stack([ac[t] ** 0.5, (1 - ac[t]) ** 0.5], 1).numpy().astype(np.float32)

    def _check_start(self, start):
        n = len(self.timesteps)
        if int(start) != start or not 0 <= start < n:
            raise ValueError("start must be an index into the %d set timesteps, got %r" % (n, start))
        return int(start)

    def edit_plan(self, num_steps, strength):
        """Audio-to-audio editing (AudioLDM style_transfer, audioldm/pipeline.py:211-239): of a schedule of `num_steps` steps only the
        last k = int(strength * num_steps) run (pipeline.py:214 t_enc), from the clip's latents noised part of the way.  Sets the
        timesteps and returns `(start, encode_timestep)`: the loop executes `timesteps[start:]` (with `coef_table(start=start)` /
        `blend_table(start=start)`), start = num_steps - k, and the clip is noised to `encode_timestep = timesteps[start - 1]`.

        That is the reference's convention, kept as it is: DDIMSampler.stochastic_encode noises to the ASCENDING index t_enc = k
        (latent_diffusion/ddim.py:246-262) while DDIMSampler.decode runs the ascending entries [:t_enc], the first of them one
        entry lower (ddim.py:280) -- the start latents carry one step more noise than the first executed timestep says.
        k = 0 would run nothing; k = num_steps indexes one past the schedule in the reference; both raise ValueError."""
        k = int(strength * num_steps)
        if not 1 <= k <= num_steps - 1:
            raise ValueError("strength %r of %d steps runs k = %d steps; an edit needs 1 <= k <= %d" % (strength, num_steps, k, num_steps - 1))
        self.set_timesteps(num_steps)
        start = num_steps - k
        return start, int(self.timesteps[start - 1])


class _SchedulerBase(_AddNoise):
    order = 1
    rule = "ddpm"

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 prediction_type="epsilon", clip_sample=True, clip_sample_range=1.0, **extra):
        if beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError("%s does is not implemented for %s" % (beta_schedule, type(self).__name__))
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError("prediction_type given as %s must be one of `epsilon`, `sample` or `v_prediction`" % prediction_type)
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      clip_sample=clip_sample, clip_sample_range=clip_sample_range, **extra)

    @classmethod
    def from_config(cls, config: dict):
        return cls(**config)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _base_timesteps(self, n):
        T = self.config.num_train_timesteps
        if n > T:
            raise ValueError(
                "`num_inference_steps`: %d cannot be larger than `self.config.train_timesteps`: %d as the unet model "
                "trained with this scheduler can only handle maximal %d timesteps." % (n, T, T))
        self.num_inference_steps = n
        ratio = T // n
        return (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64)

    def _prev(self, t):
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return t - self.config.num_train_timesteps // n


class DDPMScheduler(_SchedulerBase):
    """Stochastic DDPM sampler (what tango.py uses): scheduling_ddpm.py."""
    rule = "ddpm"

    def __init__(self, variance_type="fixed_small", **kw):
        super().__init__(variance_type=variance_type, **kw)
        self.variance_type = variance_type

    def set_timesteps(self, num_inference_steps, device=None):
        self.timesteps = torch.from_numpy(self._base_timesteps(num_inference_steps))

    def _get_variance(self, t):
        prev_t = self._prev(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        cur_beta = 1 - a_t / a_prev
        var = (1 - a_prev) / (1 - a_t) * cur_beta
        if self.variance_type == "fixed_small":
            var = torch.clamp(var, min=1e-20)
        elif self.variance_type == "fixed_large":
            var = cur_beta
        else:
            raise NotImplementedError("variance_type %s" % self.variance_type)
        return var

    def coef_table(self, start=0) -> np.ndarray:
        """[N - start, 8] fp32: sqrt(abar_t), sqrt(1-abar_t), coef_x0, coef_xt, sigma (0 at t == 0), 0, 0, 0 for the set timesteps
        from index `start` on (a one-step rule: the truncated table is rows start: of the full one)"""
        rows = []
        for t in self.timesteps.tolist()[self._check_start(start):]:
            prev_t = self._prev(t)
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
            b_t, b_prev = 1 - a_t, 1 - a_prev
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            c_x0 = (a_prev ** 0.5 * cur_b) / b_t
            c_xt = cur_a ** 0.5 * b_prev / b_t
            sig = self._get_variance(t) ** 0.5 if t > 0 else torch.tensor(0.0)
            rows.append([float(a_t ** 0.5), float(b_t ** 0.5), float(c_x0), float(c_xt), float(sig), 0.0, 0.0, 0.0])
        return np.asarray(rows, dtype=np.float32)


class DDIMScheduler(_SchedulerBase):
    """DDIM rule (fork schedulers/scheduling_ddim.py:238-360; AudioLDM's DDIMSampler.p_sample_ddim, audioldm/latent_diffusion/
    ddim.py:306-377, is the same update): the north-star's optional sampler.  `eta` = 0 (default) is the deterministic rule;
    eta > 0 adds sigma_t = eta * sqrt((1 - abar_prev) / (1 - abar_t) * (1 - abar_t / abar_prev)) of fresh noise per step and
    shortens the direction term to sqrt(1 - abar_prev - sigma_t^2) (scheduling_ddim.py:316-352, ddim.py:356-370; eta = 1 is
    DDPM-like ancestral sampling).  The noise comes from the engine's step-noise source (injected tensor or device Philox),
    like the DDPM rule's."""
    rule = "ddim"

    def __init__(self, set_alpha_to_one=True, steps_offset=0, eta=0.0, **kw):
        super().__init__(set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset, **kw)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        if eta < 0:
            raise ValueError("eta must be >= 0")
        self.eta = float(eta)

    def set_timesteps(self, num_inference_steps, device=None):
        self.timesteps = torch.from_numpy(self._base_timesteps(num_inference_steps)) + self.config.steps_offset

    def coef_table(self, eta=None, start=0) -> np.ndarray:
        """per-step coefficients of the fused update; `eta` overrides the constructor's value for this table (the fork passes eta to
        every step() call, scheduling_ddim.py:238: here the loop is one engine call, so it is a per-table argument); `start`: rows
        start: only (a truncated loop, edit_plan())"""
        eta = self.eta if eta is None else float(eta)
        if eta < 0:
            raise ValueError("eta must be >= 0")
        rows = []
        T = self.config.num_train_timesteps
        for t in self.timesteps.tolist()[self._check_start(start):]:
            prev_t = t - T // self.num_inference_steps
            a_t = self.alphas_cumprod[t]
            a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
            b_t = 1 - a_t
            var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)          # scheduling_ddim.py:184-193
            std = eta * var ** 0.5                                           # :316-317 (eta = 0 -> std_dev_t = 0)
            direction = (1 - a_prev - std ** 2) ** 0.5                       # :340
            rows.append([float(a_t ** 0.5), float(b_t ** 0.5), 0.0, 0.0, float(std), float(a_prev ** 0.5), float(direction), 0.0])
        return np.asarray(rows, dtype=np.float32)


class DDIMInverseScheduler(_SchedulerBase):
    """DDIM inversion after the fork's scheduling_ddim_inverse.py:25-268: the deterministic encoder of an edit.  The timesteps
    ASCEND (`arange(0, n) * ratio + steps_offset`, :186-208) and step() (:210-265) is the DDIM update with the NEXT abar where the
    sampler has the previous one: prev = sqrt(abar_next) * x0 + sqrt(1 - abar_next) * eps.  That is the `rule != 0` branch of the
    engine's fused step with sigma = 0, so inversion runs through Engine.denoise with `rule = "ddim"` and this class's table: no
    kernel of its own.  Past the last training timestep abar_next is `final_alpha_cumprod`: 0 with `set_alpha_to_zero` (the step
    then returns the predicted noise), else abar of the last training timestep (:157-162).

    Built on a sampler (`from_scheduler`), the grid is the SAMPLER's own, walked upward: entry 0 is the clean level (the sampler's
    `steps_offset`, 0 where it has none) and entry j >= 1 is `sampler.timesteps[N - 1 - j]`, so that k steps from clean latents
    land exactly on `sampler.edit_plan(N, k / N)`'s encode timestep `timesteps[N - k - 1]`.  For a DDIMScheduler that is the
    fork's grid above, entry for entry.  The multistep DPM-Solver's timesteps are linspace-spaced and end one spacing above the
    clean level 0 (N = 20: 999 ... 100, 50, then 0), so its inverse grid is 0, 100, 150, ...: the first inverse step spans two
    of the sampler's spacings, every later one spans one."""
    rule = "ddim"
    _sampler = None

    def __init__(self, set_alpha_to_zero=True, steps_offset=0, **kw):
        kw.pop("set_alpha_to_one", None)                  # a sampler's config (from_scheduler): not this class's switch
        kw.pop("eta", None)
        super().__init__(set_alpha_to_zero=set_alpha_to_zero, steps_offset=steps_offset, **kw)
        self.final_alpha_cumprod = torch.tensor(0.0) if set_alpha_to_zero else self.alphas_cumprod[-1]
        self.timesteps = torch.from_numpy(np.arange(0, self.config.num_train_timesteps).copy().astype(np.int64))

    @classmethod
    def from_scheduler(cls, scheduler, **override):
        """the inverse scheduler on the noise schedule of a sampler (`scheduler.config`: betas, prediction type, steps_offset)"""
        items = dict(vars(scheduler.config))
        accepted = _init_params(cls)
        cfg = {k: v for k, v in items.items() if k in accepted}
        if cfg.get("beta_schedule") not in ("linear", "scaled_linear"):
            raise NotImplementedError("DDIMInverseScheduler supports the linear and scaled_linear beta schedules")
        cfg.update(override)
        inv = cls(**cfg)
        inv._sampler = copy.deepcopy(scheduler)           # its set_timesteps() is called here: the caller's object stays as it is
        return inv

    def set_timesteps(self, num_inference_steps, device=None):
        base = self._base_timesteps(num_inference_steps)[::-1].copy() + self.config.steps_offset
        if self._sampler is not None:
            self._sampler.set_timesteps(num_inference_steps)
            ts = np.asarray(torch.as_tensor(self._sampler.timesteps).cpu().numpy()[::-1], dtype=np.int64).copy()
            ts[0] = self.config.steps_offset
            if len(ts) != num_inference_steps or np.any(np.diff(ts) <= 0):
                raise ValueError("the sampler's %d timesteps do not ascend strictly from the clean level %d: %s"
                                 % (num_inference_steps, self.config.steps_offset, ts.tolist()))
            base = ts
        self.timesteps = torch.from_numpy(base)
        # the level each step moves to: the next entry; past the last one the fork's t + T // n (:236), i.e. final_alpha_cumprod
        last = int(base[-1]) + self.config.num_train_timesteps // num_inference_steps
        self._next_timestep = dict(zip(base.tolist(), base.tolist()[1:] + [last]))

    def _next_alpha(self, t):
        nxt = self._next_timestep[t]
        return self.alphas_cumprod[nxt] if nxt < self.config.num_train_timesteps else self.final_alpha_cumprod

    def coef_table(self, count=None) -> np.ndarray:
        """[count, 8] fp32 rows sqrt(abar_t), sqrt(1 - abar_t), 0, 0, 0, sqrt(abar_next), sqrt(1 - abar_next), 0 of the first `count`
        (default: all) inverse steps, each a 0-dim fp32 torch expression in the fork's order"""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() before coef_table()")
        n = len(self.timesteps)
        count = n if count is None else int(count)
        if not 1 <= count <= n:
            raise ValueError("count must be in [1, %d], got %d" % (n, count))
        rows = []
        for t in self.timesteps.tolist()[:count]:
            a_t, a_next = self.alphas_cumprod[t], self._next_alpha(t)
            b_t = 1 - a_t
            rows.append([float(a_t ** 0.5), float(b_t ** 0.5), 0.0, 0.0, 0.0, float(a_next ** 0.5), float((1 - a_next) ** 0.5), 0.0])
        return np.asarray(rows, dtype=np.float32)

    def step(self, model_output, timestep, sample, return_dict=True, **_):
        """scheduling_ddim_inverse.py:210-265 in its expression order (torch; the engine's fused step computes the same bits)"""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        a_t, a_next = self.alphas_cumprod[t], self._next_alpha(t)
        b_t = 1 - a_t
        p = self.config.prediction_type
        if p == "epsilon":
            x0 = (sample - b_t ** 0.5 * model_output) / a_t ** 0.5
            eps = model_output
        elif p == "sample":
            x0 = model_output
            eps = (sample - a_t ** 0.5 * x0) / b_t ** 0.5
        else:
            x0 = (a_t ** 0.5) * sample - (b_t ** 0.5) * model_output
            eps = (a_t ** 0.5) * model_output + (b_t ** 0.5) * sample
        if self.config.clip_sample:
            x0 = x0.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)
        direction = (1 - a_next) ** 0.5 * eps
        prev = a_next ** 0.5 * x0 + direction
        return _StepOutput(prev) if return_dict else (prev, x0)


def _glide_cosine_betas(num_train_timesteps, max_beta=0.999):
    """"squaredcos_cap_v2": the cosine schedule of Nichol & Dhariwal (2021), abar(t) = cos((t + 0.008) / 1.008 * pi / 2)^2, as
    betas 1 - abar(t_{i+1}) / abar(t_i) clipped at `max_beta`, computed in Python floats and rounded to fp32 once"""
    import math

    def abar(x):
        return math.cos((x + 0.008) / 1.008 * math.pi / 2) ** 2

    T = num_train_timesteps
    return torch.tensor([min(1 - abar((i + 1) / T) / abar(i / T), max_beta) for i in range(T)], dtype=torch.float32)


class DPMSolverMultistepScheduler(_AddNoise):
    """Multistep DPM-Solver / DPM-Solver++ (Lu et al. 2022, arXiv 2206.00927 and 2211.01095), with the constructor, defaults and
    step semantics of the fork's scheduling_dpmsolver_multistep.py:124-495: 20-25 UNet calls instead of DDPM's 100-200.

    The update of step i is a linear combination of the current latent x, the converted model output m0 (x0 for `dpmsolver++`,
    eps for `dpmsolver`) and the converted outputs m1, m2 of the two steps before, with scalars that depend only on the schedule.
    `coef_table()` computes those scalars on the host, as the fork's own 0-dim fp32 tensor expressions, so the engine's fused
    kernel (rule 2) reproduces the fork's `step()` bit for bit; `step()` here applies the same table row in torch (the tests' reference loop,
    callers that drive their own loop).  Deterministic: there is no noise term.

    Row layout of `coef_table()` ([N, 16] fp32, include/tango_engine.h): alpha_s0, sigma_s0, kx, c0, c1, c2, 1/r0, 1/r1,
    r0/(r0+r1), 1/(r0+r1), order, algorithm (0 dpmsolver++, 1 dpmsolver), 0, 0, 0, 0.  The update is
        order 1: kx*x + c0*D0
        order 2: (kx*x + c0*D0) + c1*D1                 D1 = (1/r0)*(m0 - m1)
        order 3: ((kx*x + c0*D0) + c1*D1) + c2*D2       D1_0 = (1/r0)*(m0 - m1), D1_1 = (1/r1)*(m1 - m2),
                                                        D1 = D1_0 + (r0/(r0+r1))*(D1_0 - D1_1), D2 = (1/(r0+r1))*(D1_0 - D1_1)
    with D0 = m0; the fork's subtracted terms are stored as negated coefficients (a - k*b == a + (-k)*b exactly)."""
    order = 1
    rule = "dpmsolver"
    COEF_WIDTH = 16

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True):
        if trained_betas is not None:
            betas = torch.tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "squaredcos_cap_v2":
            betas = _glide_cosine_betas(num_train_timesteps)
        else:
            raise NotImplementedError("%s does is not implemented for %s" % (beta_schedule, type(self).__name__))
        if algorithm_type == "deis":                      # the fork's quirk: DEIS configs run as DPM-Solver++
            algorithm_type = "dpmsolver++"
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError("%s does is not implemented for %s" % (algorithm_type, type(self).__name__))
        if solver_type in ("logrho", "bh1", "bh2"):       # the fork's quirk: UniPC / DEIS solver types run as midpoint
            solver_type = "midpoint"
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError("%s does is not implemented for %s" % (solver_type, type(self).__name__))
        if solver_order not in (1, 2, 3):
            raise ValueError("solver_order must be 1, 2 or 3, got %r" % (solver_order,))
        if prediction_type not in ("epsilon", "sample", "v_prediction"):
            raise ValueError("prediction_type given as %s must be one of `epsilon`, `sample`, or `v_prediction` for the "
                             "DPMSolverMultistepScheduler." % prediction_type)
        if thresholding:
            raise NotImplementedError("thresholding=True is not supported: dynamic thresholding needs a per-sample quantile of the "
                                      "predicted x0 and is meant for pixel-space models, not this latent model")
        T = num_train_timesteps
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.alpha_t = torch.sqrt(self.alphas_cumprod)
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.init_noise_sigma = 1.0
        self.config = SimpleNamespace(num_train_timesteps=T, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                                      trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type,
                                      thresholding=False, dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                                      sample_max_value=sample_max_value, algorithm_type=algorithm_type, solver_type=solver_type,
                                      lower_order_final=lower_order_final, clip_sample=False, clip_sample_range=1.0)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, T - 1, T, dtype=np.float32)[::-1].copy())
        self.model_outputs = [None] * solver_order
        self.lower_order_nums = 0

    @classmethod
    def from_config(cls, config):
        """`config`: a dict or the `config` namespace of another scheduler (`DPMSolverMultistepScheduler.from_config(
        tango.scheduler.config)`); keys the constructor does not take are ignored"""
        items = config.items() if isinstance(config, dict) else vars(config).items()
        accepted = _init_params(cls)
        return cls(**{k: v for k, v in items if k in accepted})

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        """N + 1 points evenly spaced over [0, T-1], rounded, descending, the final 0 dropped (scheduling_dpmsolver_multistep.py:
        185-206).  The table stays on the host: the engine takes it as host data."""
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ts = np.linspace(0, T - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)
        self.model_outputs = [None] * self.config.solver_order
        self.lower_order_nums = 0

    # ---- the per-step scalars ------------------------------------------------------------------------------------------------
    def _step_order(self, i, lower_order_nums):
        """the order the fork's step() runs at loop index i (scheduling_dpmsolver_multistep.py:464-487)"""
        n = len(self.timesteps)
        short = self.config.lower_order_final and n < 15
        k = self.config.solver_order
        if k == 1 or lower_order_nums < 1 or (short and i == n - 1):
            return 1
        if k == 2 or lower_order_nums < 2 or (short and i == n - 2):
            return 2
        return 3

    def _row(self, i, order):
        """row i of the table as 0-dim fp32 tensors, each computed in the fork's expression order"""
        ts = self.timesteps
        s0 = int(ts[i])
        t = 0 if i == len(ts) - 1 else int(ts[i + 1])             # the final step targets timestep 0
        z = torch.tensor(0.0)
        lam_t, lam_s0 = self.lambda_t[t], self.lambda_t[s0]
        alpha_t, alpha_s0 = self.alpha_t[t], self.alpha_t[s0]
        sigma_t, sigma_s0 = self.sigma_t[t], self.sigma_t[s0]
        h = lam_t - lam_s0
        pp = self.config.algorithm_type == "dpmsolver++"
        heun = self.config.solver_type == "heun"
        if pp:
            kx = sigma_t / sigma_s0
            c0 = -(alpha_t * (torch.exp(-h) - 1.0))
        else:
            kx = alpha_t / alpha_s0
            c0 = -(sigma_t * (torch.exp(h) - 1.0))
        c1 = c2 = inv_r0 = inv_r1 = q = inv_r01 = z
        if order >= 2:
            lam_s1 = self.lambda_t[int(ts[i - 1])]
            h_0 = lam_s0 - lam_s1
            r0 = h_0 / h
            inv_r0 = 1.0 / r0
        if order == 2:
            if pp:
                c1 = (alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)) if heun else -(0.5 * (alpha_t * (torch.exp(-h) - 1.0)))
            else:
                c1 = -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0)) if heun else -(0.5 * (sigma_t * (torch.exp(h) - 1.0)))
        elif order == 3:
            lam_s2 = self.lambda_t[int(ts[i - 2])]
            h_1 = lam_s1 - lam_s2
            r1 = h_1 / h
            inv_r1 = 1.0 / r1
            q = r0 / (r0 + r1)
            inv_r01 = 1.0 / (r0 + r1)
            if pp:
                c1 = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
                c2 = -(alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5))
            else:
                c1 = -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0))
                c2 = -(sigma_t * ((torch.exp(h) - 1.0 - h) / h ** 2 - 0.5))
        return [alpha_s0, sigma_s0, kx, c0, c1, c2, inv_r0, inv_r1, q, inv_r01]

    def _check_distinct(self):
        ts = self.timesteps.tolist()
        if len(set(ts)) != len(ts):
            raise ValueError("the schedule of %d steps repeats a timestep (%d distinct of %d training steps): a multistep solver "
                             "cannot step between equal timesteps" % (len(ts), len(set(ts)), self.config.num_train_timesteps))

    def coef_table(self, start=0) -> np.ndarray:
        """[N - start, 16] fp32 per-step scalars of the fused update (layout: class docstring).  `start` > 0 is the table of a loop
        over `timesteps[start:]` (edit_plan()): NOT rows start: of the full table -- the loop has no history yet, so its first step
        is order 1 and the order ramp restarts, which is what the fork does when a pipeline slices `scheduler.timesteps[t_start:]`
        after a fresh set_timesteps (lower_order_nums == 0); `lower_order_final` still counts from the true end of the schedule.
        step() replays the same loop when it is first called with `timesteps[start]`."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps() before coef_table()")
        self._check_distinct()
        start = self._check_start(start)
        algo = 0.0 if self.config.algorithm_type == "dpmsolver++" else 1.0
        rows = []
        for i in range(start, len(self.timesteps)):
            order = self._step_order(i, min(i - start, self.config.solver_order))
            rows.append([float(v) for v in self._row(i, order)] + [float(order), algo, 0.0, 0.0, 0.0, 0.0])
        return np.asarray(rows, dtype=np.float32)

    # ---- torch step (the tests' reference loop, callers that drive their own loop) ----------------------------------------------
    def convert_model_output(self, model_output, timestep, sample):
        """x0 (dpmsolver++) or eps (dpmsolver) from the model's prediction (scheduling_dpmsolver_multistep.py:220-281)"""
        a, s = self.alpha_t[timestep], self.sigma_t[timestep]
        p = self.config.prediction_type
        if self.config.algorithm_type == "dpmsolver++":
            if p == "epsilon":
                return (sample - s * model_output) / a
            if p == "sample":
                return model_output
            return a * sample - s * model_output
        if p == "epsilon":
            return model_output
        if p == "sample":
            return (sample - a * model_output) / s
        return a * model_output + s * sample

    def step(self, model_output, timestep, sample, return_dict=True):
        """one multistep update; keeps the fork's state (`model_outputs`, `lower_order_nums`) between calls"""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        hit = (self.timesteps == int(timestep)).nonzero()
        if len(hit) > 1:
            raise ValueError("timestep %d occurs %d times in the schedule" % (int(timestep), len(hit)))
        i = len(self.timesteps) - 1 if len(hit) == 0 else int(hit[0, 0])
        order = self._step_order(i, self.lower_order_nums)
        alpha_s0, sigma_s0, kx, c0, c1, c2, inv_r0, inv_r1, q, inv_r01 = self._row(i, order)
        m0 = self.convert_model_output(model_output, int(self.timesteps[i]), sample)
        self.model_outputs = self.model_outputs[1:] + [m0]
        x = kx * sample + c0 * m0
        if order == 2:
            x = x + c1 * (inv_r0 * (m0 - self.model_outputs[-2]))
        elif order == 3:
            m1, m2 = self.model_outputs[-2], self.model_outputs[-3]
            d10, d11 = inv_r0 * (m0 - m1), inv_r1 * (m1 - m2)
            x = (x + c1 * (d10 + q * (d10 - d11))) + c2 * (inv_r01 * (d10 - d11))
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        return _StepOutput(x) if return_dict else (x,)


_FROM_DIFFUSERS = {"DDPMScheduler": DDPMScheduler, "DDIMScheduler": DDIMScheduler, "DDIMInverseScheduler": DDIMInverseScheduler,
                   "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler}


def from_diffusers(obj):
    """the engine's scheduler for a diffusers (or fork) scheduler object, chosen by class name and built from `obj.config`; the
    engine's own scheduler objects are returned as they are"""
    if hasattr(obj, "coef_table"):
        return obj
    name = type(obj).__name__
    cls = _FROM_DIFFUSERS.get(name)
    if cls is None:
        raise TypeError("cannot run a %s on the engine: supported schedulers are %s" % (name, ", ".join(sorted(_FROM_DIFFUSERS))))
    cfg = obj.config
    items = dict(cfg.items()) if hasattr(cfg, "items") else dict(vars(cfg))
    if cls is not DPMSolverMultistepScheduler:
        if items.get("thresholding"):
            raise NotImplementedError("thresholding=True is not supported by the engine's %s" % name)
        if items.get("trained_betas") is not None:
            raise NotImplementedError("trained_betas is not supported by the engine's %s" % name)
    accepted = _init_params(cls)
    return cls(**{k: v for k, v in items.items() if k in accepted})


def _init_params(cls):
    """the named constructor parameters of `cls` and its bases"""
    import inspect
    names = set()
    for c in cls.__mro__:
        if "__init__" in vars(c) and c is not object:
            names |= {p.name for p in inspect.signature(c.__init__).parameters.values()
                      if p.kind not in (p.VAR_KEYWORD, p.VAR_POSITIONAL)}
    return names - {"self"}


# ---- guidance as a table (include/tango_engine.h tango_guidance_args_t) ------------------------------------------------------------
def guidance_is_table(guidance):
    """False for a plain scalar (a Python / numpy number or a 0-dim array / tensor), True for a sequence, array or tensor"""
    if torch.is_tensor(guidance):
        return guidance.dim() > 0
    return np.ndim(guidance) > 0


def cfg_enabled(guidance):
    """does this guidance argument run the [uncond; cond] batch?  A scalar: when > 1 (models.py:213); a table: always"""
    return True if guidance_is_table(guidance) else float(guidance) > 1.0


def guidance_table(guidance, num_steps, batch):
    """The host table of a guidance argument: None for a plain scalar (the engine's scalar path, unchanged), else float32
    [num_steps, batch] -- a [batch] row (one scale per latents row, constant over the steps) repeated for every step, or a
    [num_steps, batch] schedule as it is.  `batch` counts latents rows (prompts x samples).  ValueError for any other shape and for
    entries that are negative or not finite (1.0 gives the conditional output, 0.0 the unconditional one)."""
    if not guidance_is_table(guidance):
        return None
    g = guidance.detach().cpu().numpy() if torch.is_tensor(guidance) else np.asarray(guidance)
    g = g.astype(np.float32)
    if g.shape == (batch,):
        g = np.broadcast_to(g, (num_steps, batch))
    elif g.shape != (num_steps, batch):
        raise ValueError("a guidance table is [%d] (per sample) or [%d, %d] (per step and sample), got %s"
                         % (batch, num_steps, batch, g.shape))
    if not np.all(np.isfinite(g)) or np.any(g < 0):
        raise ValueError("guidance table entries must be finite and >= 0")
    return np.ascontiguousarray(g)


def check_guidance_rescale(guidance, guidance_rescale):
    """guidance_rescale in [0, 1], and > 0 only with classifier-free guidance on: ValueError otherwise (no device needed)"""
    r = float(guidance_rescale)
    if not 0.0 <= r <= 1.0:          # NaN fails both comparisons
        raise ValueError("guidance_rescale must be in [0, 1], got %r" % (guidance_rescale,))
    if r > 0.0 and not cfg_enabled(guidance):
        raise ValueError("guidance_rescale needs classifier-free guidance: guidance > 1 or a guidance table, got %r" % (guidance,))
    return r
