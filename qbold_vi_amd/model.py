"""Encoder, reparameterised sampling and the variational objective -- host mirror of the
reference's model.py (ReparamTrickLayer :15-50, EncoderTrainer :53-770).

Class and method names, argument order and defaults follow the reference; tensors are float32
ROCm tensors, channel-last, with the mask carried as the LAST channel of the "true" tensors
exactly as Keras hands them to the reference's loss callables.  Voxel batches may have any leading
shape; the reference's 5-D (B, X, Y, Z, C) layout is accepted as is.  Arithmetic is done by
libqbold_hip.so; torch provides memory, reshapes and trivial reductions of kernel outputs.

Scope: the branches optimal.yaml disables are built where the reference itself can run them (population
prior / MoG / inverse-gamma with the diagonal family, dropout and GroupNorm on the layer-wise kernels); the pairs the
reference cannot evaluate raise NotImplementedError instead of silently computing something else.  Image crops [B, X, Y, Z, C]
 take the layer-wise spatial kernels; voxel batches the fused ones.
"""
import math

import numpy as np
import torch

from .init import init_encoder_weights
from .ops import Context, EncoderWeights


def _pad5(t):
    """Distribution parameters as the kernels take them: 5 per voxel.  The diagonal family
    (use_mvg=False, model.py:33-37) is the 5-parameter one with a zero Cholesky term."""
    if t.shape[-1] == 5:
        return t
    if t.shape[-1] == 8:   # infer_inv_gamma: [4 parameters | 4 hyper-parameters] (model.py:205): the parameters
        t = t[..., :4]
    if t.shape[-1] != 4:
        raise ValueError("distribution parameters must have 4 (use_mvg=False) or 5 channels")
    return torch.cat([t, torch.zeros_like(t[..., :1])], -1)


def _flat(t, c):
    return t.reshape(-1, c)


R2P_LOSS_SAMPLES = 10   # n_samples of the R2' term, model.py:479

class EncoderModel:
    """Stands in for the Keras `outer_model` of create_encoder (model.py:222): model(x) ->
    [out1 (stream 1, [...,5]), out2 (stream 2, [...,5]), sigma ([...,T])]."""

    def __init__(self, trainer, weights):
        self._trainer = trainer
        self.weights = weights
        # infer_inv_gamma (model.py:201-205): a tfp VariableLayer of four exp-activated scalars -- the inverse-gamma
        # (alpha, beta) of the OEF and DBV variances -- initialised to log([20, 2.5, 20, 2.5]) and appended to the
        # first output as constant channels.  Host state (four numbers): hyper_raw holds the logs.
        self.hyper_raw = np.log(np.array([20.0, 2.5, 20.0, 2.5])) if trainer._infer_inv_gamma else None

    def hyper_params(self):
        return np.exp(self.hyper_raw)

    def __call__(self, x):
        return self.predict(x)

    def _with_hyper(self, o1):
        if o1 is None or self.hyper_raw is None:
            return o1
        h = torch.as_tensor(self.hyper_params(), dtype=o1.dtype, device=o1.device)
        return torch.cat([o1, h.expand(o1.shape[:-1] + (4,))], -1)   # model.py:205

    def predict(self, x, want=("out1", "out2", "sigma")):
        """Voxel batches go through the fused kernels; image crops [B, X, Y, Z, T] (X or Y > 1) get
        stream 2 with its 3x3x1 'same' convolutions (stream 1 is voxel-wise by construction)."""
        ctx = self._trainer._ctx
        nq = self._trainer._nq
        cut = (lambda t: t if t is None or nq == 5 else t[..., :nq].contiguous())
        if not self._trainer._is_spatial(x):
            o1, o2, sg = ctx.encoder_fwd(self.weights, x, want=want)
            return [self._with_hyper(cut(o1)), cut(o2), sg]
        o1 = self._with_hyper(cut(ctx.encoder_fwd(self.weights, x, want=("out1",))[0])) if "out1" in want else None
        o2 = sg = None
        if "out2" in want or "sigma" in want:
            st = self._trainer._spatial_state(self.weights)
            q, ls = st.forward_spatial(x)
            o2 = cut(q.reshape(x.shape[:-1] + (5,))) if "out2" in want else None
            sg = ctx.transform("exp", ls).reshape(x.shape) if "sigma" in want else None
        return [o1, o2, sg]

    # Weights travel as .npz with the canonical tensor names (Keras HDF5 is SURVEY N3).
    def get_weights(self):
        w = self.weights.to_arrays()
        if self._trainer._nq == 4:  # the reference's final layer has 4 outputs (model.py:191-196)
            w["Wf"], w["bf"] = w["Wf"][:, :4].copy(), w["bf"][:4].copy()
        if self.hyper_raw is not None:
            w["hyper_prior"] = np.asarray(self.hyper_raw, np.float32)
        return w

    def set_weights(self, arrays):
        arrays = dict(arrays)
        if "hyper_prior" in arrays:
            hp = np.asarray(arrays.pop("hyper_prior"), np.float64)
            if self.hyper_raw is not None:
                self.hyper_raw = hp
        if np.asarray(arrays["Wf"]).shape[-1] == 4:
            Wf, bf = np.asarray(arrays["Wf"], np.float32), np.asarray(arrays["bf"], np.float32)
            arrays["Wf"] = np.concatenate([Wf, np.zeros_like(Wf[:, :1])], 1)
            arrays["bf"] = np.concatenate([bf, np.zeros(1, np.float32)])
        self.weights.set_from_arrays(arrays)

    def save_weights(self, path):
        if str(path).endswith((".h5", ".hdf5")):   # Keras layout; needs h5py (keras_h5.py)
            from .keras_h5 import save_keras_h5
            return save_keras_h5(path, self.get_weights())
        np.savez(path, **self.get_weights())

    def load_weights(self, path):
        if str(path).endswith((".h5", ".hdf5")):
            from .keras_h5 import load_keras_h5
            return self.set_weights(load_keras_h5(path))
        with np.load(path) as f:
            self.set_weights({k: f[k] for k in f.files})


class _InnerModel:
    """create_encoder also returns the `inner_model` that starts after the first 1x1x1 layer
    (model.py:217); nothing on the hot path calls it."""

    def __call__(self, *a, **k):
        raise NotImplementedError("inner_model (post-first-layer features in) is not part of the "
                                  "accelerated voxel path")


class ReparamTrickLayer:
    """Draws (OEF, DBV) samples from the predicted logit-Normal (model.py:15-50).  The normals
    come from the library's Philox stream (qbold_normals) unless `z` is given."""

    def __init__(self, encoder_trainer):
        self._encoder_trainer = encoder_trainer
        self._draws = 0

    def __call__(self, inputs, z=None):
        return self.call(inputs, z=z)

    def call(self, inputs, z=None, *args, **kwargs):
        input, mask = inputs
        tr = self._encoder_trainer
        # use_mvg=False (model.py:33-37): independent draws = the Cholesky form with a zero off-diagonal
        q = _pad5(_flat(input, input.shape[-1])[:, :tr._nq]).contiguous()
        if z is None:
            z = tr._ctx.normals(q.shape[0], 1, stream_id=0, seed=tr._seed + 104729 * self._draws)
            self._draws += 1
        return tr._ctx.reparam(q, z.reshape(-1, 2)).reshape(input.shape[:-1] + (2,))


class FineTuner:
    """The `full_model` of build_fine_tuner (model.py:239-286): full_model([data, mask]) ->
    {'predictions': q [...,5], 'predicted_images': concat[signal, sigma] [S*...,2T]}."""

    def __init__(self, trainer, encoder_model, signal_generation_layer):
        self._trainer = trainer
        self.encoder_model = encoder_model
        self.signal_generation_layer = signal_generation_layer
        self._rpl = ReparamTrickLayer(trainer)
        # heteroscedastic_noise=False (model.py:277-281): ONE exp-activated scalar, a variable of the fine-tuner
        # (not of the encoder: the weight files do not carry it), initial value log(initial_im_sigma)
        self.log_sigma = None if trainer._heteroscedastic_noise else math.log(float(trainer._initial_im_sigma))
        # use_population_prior with the diagonal family (model.py:262-271): a 4-vector variable of the fine-tuner,
        # [mu_oef, raw_s_oef, mu_dbv, raw_s_dbv], appended to 'predictions' as constant channels
        # (mog_components > 1: 4 M values, random-normal initialised, model.py:262-266)
        M = int(trainer._mog_components)
        self.pop_prior = None
        if trainer._use_population_prior:
            self.pop_prior = (np.array([-0.97, 0.4, -1.14, 0.6], np.float32) if M <= 1 else
                              np.random.default_rng(trainer._seed).standard_normal(4 * M).astype(np.float32))

    def __call__(self, inputs):
        return self.predict(inputs)

    def predict(self, inputs):
        data, mask = inputs
        tr = self._trainer
        _, q, sigma = self.encoder_model.predict(data, want=("out2", "sigma"))
        S = tr._no_samples
        qs = torch.cat([q] * S, 0)          # model.py:245
        sig = torch.cat([sigma] * S, 0)     # model.py:246
        sampled = self._rpl((qs, mask))     # model.py:248
        if self.pop_prior is not None:      # model.py:268-270
            pp = torch.as_tensor(self.pop_prior, device=qs.device)
            qs = torch.cat([qs, pp.expand(qs.shape[:-1] + (pp.numel(),))], -1)
        output = self.signal_generation_layer(sampled)  # model.py:273
        if self.log_sigma is not None:      # model.py:277-281: one channel holding the scalar sigma
            sig = torch.full(output.shape[:-1] + (1,), math.exp(self.log_sigma), dtype=output.dtype,
                             device=output.device)
        # 'predictions' is the S-fold tiled distribution, as in the reference (model.py:245,285)
        return {'predictions': qs, 'predicted_images': torch.cat([output, sig], -1)}

    def elbo(self, data, mask, prior, no_samples=None, kl_samples=70, seed=1, voxel0=0, kl_tiled=None, q=None):
        """The fused path: one launch for encoder + S draws + forward model + NLL + K-draw KL
        (image crops: spatial encoder, then the ELBO kernel).
        Returns dict(nll, kl, elbo (= nll + kl, train.py:351), sums, q, nll_kl).

        kl_tiled (default: the trainer's setting, True = the reference's behaviour): with no_samples = S > 1 the
        reference tiles the batch S-fold (model.py:245-246, 656) and kl_loss draws `kl_samples` KL samples per TILED
        row, i.e. S * kl_samples draws per voxel, averaged (model.py:592-610, 661-663).  The kernels never tile; the
        same estimator is S * kl_samples in-kernel draws per voxel.  kl_tiled=False draws kl_samples per voxel
        whatever S (same expectation, S times fewer draws: round 1's behaviour).

        q (this package's addition): heads [..., C] to score instead of the encoder's (refine()'s output, say), with
        the encoder's sigma head or the fine tuner's homoscedastic sigma; None scores the encoder's heads."""
        tr = self._trainer
        S = tr._no_samples if no_samples is None else no_samples
        kl_samples = tr.kl_draws(kl_samples, S, kl_tiled)
        x = _flat(data, data.shape[-1])
        m = None if mask is None else mask.reshape(-1)
        p5 = _pad5(_flat(prior, prior.shape[-1])).contiguous()
        K = kl_samples if tr._use_mvg else 0   # diagonal family: closed-form KL below (model.py:686-716)
        mog = self.pop_prior is not None and self.pop_prior.size > 4
        if self.pop_prior is not None and not mog:   # the per-voxel prior is ignored (model.py:687-690): one population prior
            p5 = _pad5(torch.as_tensor(self.pop_prior, device=x.device).expand(x.shape[0], 4)).contiguous()
        if q is not None or tr._is_spatial(data) or self.log_sigma is not None:
            _, q5, sg5 = self.encoder_model.predict(data, want=("out2", "sigma"))
            q = _pad5(_flat(q5 if q is None else q, q5.shape[-1])).contiguous()
            sg = _flat(sg5, x.shape[-1])
            if self.log_sigma is not None:   # the encoder's sigma head is not part of this model (model.py:277-281)
                sg = torch.full_like(sg, math.exp(self.log_sigma))
            sums, nll_kl = tr._ctx.elbo_fwd(x, m, q, p5, sg, S, K, seed=seed, voxel0=voxel0)
        else:
            # range_check: activations beyond the f16 operand split's 65504 show as non-finite sums and are
            # recomputed on the exact-float32 layer-wise path (ops.Context.vi_fwd)
            sums, q, nll_kl = tr._ctx.vi_fwd(self.encoder_model.weights, x, m, p5, S, K, seed=seed, voxel0=voxel0,
                                             range_check=True)
        if not tr._use_mvg and mog:   # model.py:666-685: one draw per dimension against the mixture (no prior cost)
            # The reference tiles the batch S-fold before this loss (model.py:245-246, 656), so a voxel is scored at S
            # independent draws and their mean enters the masked sum; copy s of voxel i is row s * N + i of the tiled
            # batch, which is the Philox key kl_loss() gives it.  kl_tiled=False: one draw per voxel.
            comps = torch.as_tensor(self.pop_prior, device=x.device).reshape(-1, 4)
            tiled = tr._kl_tiled if kl_tiled is None else kl_tiled
            copies = max(int(S), 1) if tiled else 1
            kl_v = tr._ctx.kl_mog(q, comps, seed=seed, voxel0=voxel0)
            for s in range(1, copies):
                kl_v = kl_v + tr._ctx.kl_mog(q, comps, seed=seed, voxel0=voxel0 + s * x.shape[0])
            kl_v = kl_v / copies
            live = kl_v if m is None else torch.where(m > 0, kl_v, torch.zeros_like(kl_v))
            sums[1] = live.sum(dtype=torch.float64)
            nll_kl[:, 1] = kl_v
            q = q[:, :4].contiguous()
        elif not tr._use_mvg:
            ksums, kl_v = tr._ctx.kl_diag(q, p5, m)
            sums[1] = ksums[1]
            nll_kl[:, 1] = kl_v
            q = q[:, :4].contiguous()
            if self.pop_prior is not None:   # model.py:710-716: the hyper-prior's cost joins the KL numerator
                sums[1] = sums[1] + tr.population_prior_cost(self.pop_prior, data.shape[0])
        return dict(sums=sums, q=q, nll_kl=nll_kl, nll=sums[0] / sums[2], kl=sums[1] / sums[2],
                    elbo=(sums[0] + sums[1]) / sums[2])

    def log_evidence(self, data, mask, prior, no_samples=100, seed=1, voxel0=0, want_means=False, q=None, psis=False,
                     psis_chunk=None):
        """Importance-weighted evidence (Burda et al. 2016) of `no_samples` = K draws per voxel from the fitted
        posterior, on the encoder heads of encoder_model.predict (as the spatial branch of elbo() takes them) and the
        homoscedastic sigma when the fine tuner carries one.  Per voxel, shaped like the data's spatial dims:
          log_evidence  log p^ = logsumexp_k log w_k - log K  (>= elbo; -> log p(x) as K grows)
          elbo          mean_k log w_k: the ELBO of the SAME draws (log w = -nll - log q + log prior)
          ess           (sum w)^2 / sum w^2 in [1, K]: how well q covers the posterior
          is_means      [..., 3] self-normalised posterior means of (OEF, DBV, R2') (want_means) or None
        and the masked sums (distributed.allreduce_sums reduces them across shards) with mean_log_evidence,
        mean_elbo and gap = mean_log_evidence - mean_elbo (an estimate of the mean KL(q || p(z | x))).
        q: heads [..., 5] to evaluate instead of the encoder's (refine()'s output, say); sigma as above.
        psis=True (needs 25 <= no_samples <= 1024): Pareto-smoothed importance sampling (Vehtari et al. 2024) of the
        SAME draws (Context.log_evidence_draws + Context.psis), which adds
          khat               the tail shape k^ of the voxel's weights: the estimates above are reliable below
                             khat_threshold = min(1 - 1 / log10 K, 0.7); above 0.7 no K will save them
          log_evidence_psis  log p^ from the smoothed weights
          ess_psis           1 / sum w~^2 of the smoothed normalised weights
          psis_means         [..., 3] the smoothed-weight means of (OEF, DBV, R2')
        (NaN outside the mask), computed in voxel chunks whose per-draw buffers stay under 256 MiB (psis_chunk: voxels
        per chunk instead); chunks pass their own voxel0, so the result does not depend on the chunking."""
        from .distributed import log_evidence_from_sums
        if psis and not 25 <= int(no_samples) <= 1024:   # QBOLD_PSIS_MIN_K, QBOLD_PSIS_MAX_K
            raise ValueError("log_evidence(psis=True) needs 25 <= no_samples <= 1024")
        tr = self._trainer
        self._check_mvn_family("log_evidence")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        sums, out, means = tr._ctx.log_evidence(x, m, q, p5, sg, no_samples, seed=seed, voxel0=voxel0,
                                                want_means=want_means)
        lead = data.shape[:-1]
        lp, el, gap = log_evidence_from_sums(sums)
        res = dict(log_evidence=out[:, 0].reshape(lead), elbo=out[:, 1].reshape(lead), ess=out[:, 2].reshape(lead),
                   is_means=None if means is None else means.reshape(lead + (3,)), sums=sums,
                   mean_log_evidence=lp, mean_elbo=el, gap=gap)
        if psis:
            from .ops import psis_khat_threshold
            K, N = int(no_samples), x.shape[0]
            chunk = int(psis_chunk) if psis_chunk else max((256 << 20) // (16 * K) - 1, 1)   # log_w + theta: 16 K bytes
            if chunk < 1:
                raise ValueError("psis_chunk must be positive")
            po = torch.empty((N, 4), dtype=torch.float32, device=x.device)
            pm = torch.empty((N, 3), dtype=torch.float32, device=x.device)
            for a in range(0, N, chunk):
                b = min(a + chunk, N)
                mc = None if m is None else m[a:b]
                lw, th = tr._ctx.log_evidence_draws(x[a:b], mc, q[a:b], p5[a:b], sg[a:b], K, seed=seed,
                                                    voxel0=voxel0 + a, want_theta=True)
                po[a:b], pm[a:b], _ = tr._ctx.psis(lw, th, mc)
            res.update(khat=po[:, 0].reshape(lead), log_evidence_psis=po[:, 1].reshape(lead),
                       ess_psis=po[:, 2].reshape(lead), psis_means=pm.reshape(lead + (3,)),
                       khat_threshold=psis_khat_threshold(K))
        return res

    def credible_intervals(self, data, mask, prior, q=None, no_samples=256, psis=True, probs=(0.025, 0.5, 0.975),
                           hpd_mass=0.95, seed=1, voxel0=0, psis_chunk=None):
        """The uncertainty of the importance-corrected posterior per voxel, from the `no_samples` = K draws of
        log_evidence() for the same seed and voxel0 (Context.log_evidence_draws), weighted by their Pareto-smoothed
        importance weights (psis=True: Context.psis(want_weights=True), 25 <= K <= 1024) or by the raw ones
        (psis=False, 4 <= K <= 1024), and summarised by Context.draw_summary.  Shaped like the data's spatial dims, for
        (OEF, DBV, R2') along the axis of 3:
          mean, sd      [..., 3] the weighted moments
          quantiles     [..., 3, P] at `probs`, by the inverse weighted ECDF: each is one of the draws
          hpd           [..., 3, 2] the shortest interval that holds hpd_mass
          corr_oef_dbv  the weighted correlation of OEF and DBV
          ess           1 / sum w~^2 of the weights used
          khat          (psis) the tail shape k^ of the voxel's raw weights; khat_threshold beside it
        NaN outside the mask.  q: heads [..., 5] instead of the encoder's (refine() / laplace() / adapt() output).
        Computed in voxel chunks by log_evidence(psis=True)'s rule (per-draw buffers under 256 MiB, or psis_chunk
        voxels); chunks pass their own voxel0, so the result does not depend on the chunking."""
        K = int(no_samples)
        if psis and not 25 <= K <= 1024:   # QBOLD_PSIS_MIN_K, QBOLD_PSIS_MAX_K
            raise ValueError("credible_intervals(psis=True) needs 25 <= no_samples <= 1024")
        if not 4 <= K <= 1024:   # QBOLD_SUMMARY_MIN_K, QBOLD_SUMMARY_MAX_K
            raise ValueError("credible_intervals needs 4 <= no_samples <= 1024")
        tr = self._trainer
        self._check_mvn_family("credible_intervals")
        T = data.shape[-1]
        x = _flat(data, T)
        N = x.shape[0]
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        probs = tuple(float(p) for p in probs)
        P = len(probs)
        chunk = int(psis_chunk) if psis_chunk else max((256 << 20) // (16 * K) - 1, 1)   # log_w + theta: 16 K bytes
        if chunk < 1:
            raise ValueError("psis_chunk must be positive")
        new = lambda *s: torch.empty((N,) + s, dtype=torch.float32, device=x.device)   # noqa: E731
        stats, quant, row_out, corr = new(3, 4), new(3, P), new(2), new(3)
        khat = new() if psis else None
        for a in range(0, N, chunk):
            b = min(a + chunk, N)
            mc = None if m is None else m[a:b]
            lw, th = tr._ctx.log_evidence_draws(x[a:b], mc, q[a:b], p5[a:b], sg[a:b], K, seed=seed, voxel0=voxel0 + a,
                                                want_theta=True)
            if psis:
                po, _, lw = tr._ctx.psis(lw, None, mc, want_weights=True)
                khat[a:b] = po[:, 0]
            st, qt, ro, cr = tr._ctx.draw_summary(th, lw, mc, probs=probs, hpd_mass=hpd_mass, want_corr=True)
            stats[a:b], row_out[a:b], corr[a:b] = st, ro, cr
            if P:
                quant[a:b] = qt
        lead = data.shape[:-1]
        res = dict(mean=stats[..., 0].reshape(lead + (3,)), sd=stats[..., 1].reshape(lead + (3,)),
                   quantiles=quant.reshape(lead + (3, P)), hpd=stats[..., 2:4].reshape(lead + (3, 2)),
                   corr_oef_dbv=corr[:, 0].reshape(lead), ess=row_out[:, 0].reshape(lead), probs=probs)
        if psis:
            from .ops import psis_khat_threshold
            res.update(khat=khat.reshape(lead), khat_threshold=psis_khat_threshold(K))
        return res

    def _check_mvn_family(self, what):
        if not self._trainer._use_mvg:
            raise NotImplementedError(
                f"{what} works on the use_mvg=True family (the logit-MVN of transform_std / transform_offdiag); "
                "the diagonal family draws with exp(raw_s), not transform_std (model.py:696-698), so it is a "
                "different density")
        if self.pop_prior is not None:
            raise NotImplementedError(f"{what} needs a per-voxel prior; the population prior is not built for it")

    def _heads_and_sigma(self, data, q=None):
        """Flat heads [N, 5] (the encoder's, or the given q) and the sigma [N, T] that goes with them: the encoder's
        sigma head, or the fine tuner's homoscedastic sigma when it carries one."""
        T = data.shape[-1]
        _, q5, sg5 = self.encoder_model.predict(data, want=("out2", "sigma"))
        q = _flat(q5 if q is None else torch.as_tensor(q, device=q5.device), q5.shape[-1]).contiguous()
        sg = _flat(sg5, T)
        if self.log_sigma is not None:   # the encoder's sigma head is not part of this model (model.py:277-281)
            sg = torch.full_like(sg, math.exp(self.log_sigma))
        return q, sg

    def calibration(self, data, theta_true, mask=None, prior=None, no_samples=255, q=None, psis=False, seed=1, voxel0=0,
                    bins=16, psis_chunk=None):
        """Calibration of the posteriors against a KNOWN truth (Context.calibration; simulation-based calibration, Talts
        et al. 2018): theta_true [..., 2] = the (OEF, DBV) that generated `data`, the heads q [..., 5] (None: the encoder
        heads of encoder_model.predict; refine()'s output, say), `no_samples` = L draws per voxel -- the draws of
        log_evidence() for the same seed and voxel0.  Returns dict(out [..., 6] = (pit_oef, pit_dbv, hpd, rank
        fractions of OEF, DBV, R2'), khat (psis) or None, summary = calibration.summarise(out, L, bins): histograms,
        uniformity chi-square and interval coverage).  Voxels outside the mask are NaN and not counted.
        psis=True (needs `prior` and 25 <= no_samples <= 1024): the ranks are taken under the Pareto-smoothed importance
        weights of those same draws (Context.log_evidence_draws + Context.psis(want_weights=True)), i.e. they test the
        importance-corrected posterior instead of q; khat [...] is each voxel's k^ and the summary carries the table
        restricted to khat below ops.psis_khat_threshold(L) as well.  Computed in voxel chunks by log_evidence(psis=True)'s
        rule (per-draw buffers under 256 MiB, or psis_chunk voxels); chunks pass their own voxel0, so the result does
        not depend on the chunking."""
        from .calibration import summarise
        tr = self._trainer
        self._check_mvn_family("calibration")
        L = int(no_samples)
        if psis and not 25 <= L <= 1024:   # QBOLD_PSIS_MIN_K, QBOLD_PSIS_MAX_K
            raise ValueError("calibration(psis=True) needs 25 <= no_samples <= 1024")
        if psis and prior is None:
            raise ValueError("calibration(psis=True) needs the prior the importance weights are taken against")
        T = data.shape[-1]
        x = _flat(data, T)
        N = x.shape[0]
        m = None if mask is None else mask.reshape(-1)
        q, sg = self._heads_and_sigma(data, q)
        th = _flat(torch.as_tensor(theta_true, device=x.device), 2).contiguous()
        lead = data.shape[:-1]
        khat = None
        if not psis:
            out = tr._ctx.calibration(th, q, m, L=L, seed=seed, voxel0=voxel0)
        else:
            p5 = _flat(prior, prior.shape[-1]).contiguous()
            chunk = int(psis_chunk) if psis_chunk else max((256 << 20) // (16 * L) - 1, 1)
            if chunk < 1:
                raise ValueError("psis_chunk must be positive")
            out = torch.empty((N, 6), dtype=torch.float32, device=x.device)
            khat = torch.empty(N, dtype=torch.float32, device=x.device)
            for a in range(0, N, chunk):
                b = min(a + chunk, N)
                mc = None if m is None else m[a:b]
                lw, _ = tr._ctx.log_evidence_draws(x[a:b], mc, q[a:b], p5[a:b], sg[a:b], L, seed=seed, voxel0=voxel0 + a)
                po, _, wts = tr._ctx.psis(lw, None, mc, want_weights=True)
                khat[a:b] = po[:, 0]
                out[a:b] = tr._ctx.calibration(th[a:b], q[a:b], mc, L=L, log_w=wts, seed=seed, voxel0=voxel0 + a)
        summary = summarise(out, L, bins=bins, weighted=psis, khat=khat)
        return dict(out=out.reshape(lead + (6,)), khat=None if khat is None else khat.reshape(lead), summary=summary)

    def refine(self, data, mask, prior, steps=200, no_samples=1, lr=0.1, lr_final=None, optimizer="adam",
               seed=1, voxel0=0, smoothness_weight=0.0, q=None):
        """Semi-amortised inference (Kim et al. 2018; Cremer et al. 2018): start from the encoder heads of
        encoder_model.predict (as log_evidence() takes them; or from given heads q [..., 5], laplace()'s say: the best
        Gaussian under the ELBO from the Laplace fit) and run `steps` Adam / SGD steps on each voxel's own
        E_q[nll] + KL(q || prior), `no_samples` likelihood draws per step, sigma held fixed (the encoder's sigma head
        or the fine tuner's homoscedastic sigma), no TV term (Context.refine_posterior; lr_final None = lr / 10).
        Voxels outside the mask keep the encoder's heads.  Returns dict(q = refined raw heads shaped like the data's
        spatial dims + (5,), loss = [..., 2] (-ELBO estimate at the first step, its mean over the last tenth of the
        steps)); q goes unchanged to calculate_means, elbo(q=...), log_evidence(q=...).
        smoothness_weight > 0 (image data [B, X, Y, Z, T] only): refine the volume under the fine-tuning loss's TV
        prior as well, full-batch steps on sum(E_q[nll] + KL) + smoothness_weight TV (Context.refine_posterior_spatial;
        the configuration's smoothness_weight gives the reference's weighting); 0 is the per-voxel refinement.
        Any tau grid of 1 to 64 points: the reference's 11 / 24 taus take the kernels specialised for them, every other
        grid the run-time-T kernels (Context.refine_posterior's kernel="auto")."""
        tr = self._trainer
        self._check_mvn_family("refine")
        T = data.shape[-1]
        smoothness_weight = float(smoothness_weight)
        if smoothness_weight != 0.0 and data.dim() != 5:
            raise ValueError("refine: smoothness_weight > 0 needs image data [B, X, Y, Z, T] (the TV term needs its "
                             f"geometry); got shape {tuple(data.shape)}")
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        lead = data.shape[:-1]
        if smoothness_weight != 0.0:
            q_out, loss = tr._ctx.refine_posterior_spatial(
                x.reshape(lead + (T,)), m, q.reshape(lead + (5,)), p5.reshape(lead + (5,)), sg.reshape(lead + (T,)),
                smoothness_weight, steps=steps, S=no_samples, lr=lr, lr_final=lr_final, optimizer=optimizer,
                seed=seed, voxel0=voxel0, want_loss=True)
            return dict(q=q_out, loss=loss)
        q_out, loss = tr._ctx.refine_posterior(x, m, q, p5, sg, steps=steps, S=no_samples, lr=lr,
                                               lr_final=lr_final,
                                               optimizer=optimizer, seed=seed, voxel0=voxel0, want_loss=True)
        return dict(q=q_out.reshape(lead + (5,)), loss=loss.reshape(lead + (2,)))

    def posterior_grid(self, data, mask, prior, q=None, **grid_kw):
        """Exact per-voxel posteriors by quadrature on the logit plane (Context.posterior_grid; grid_kw: coarse, fine,
        locate, gh, span, cut, levels, want_box), for the heads q [..., 5] (None: the encoder heads of
        encoder_model.predict, as log_evidence() takes them) and the sigma that goes with them.  Shaped like the
        data's spatial dims:
          log_evidence, elbo (exact ELBO of q), gap = log_evidence - elbo (the exact KL(q || p(z | x)))
          oef, dbv, r2p and oef_sd, dbv_sd, r2p_sd (posterior means and sds), corr (OEF-DBV posterior correlation)
          oef_ci, dbv_ci [..., 2] (credible intervals at `levels`), map [..., 2] (OEF, DBV at the grid's maximum)
          edge_mass, quad_err (large: the grid truncated / under-resolved the posterior), box [..., 4] or None
        and the masked sums (distributed.allreduce_sums reduces them across shards) with mean_log_evidence,
        mean_elbo and gap (mean_log_evidence - mean_elbo).  Voxels outside the mask are NaN."""
        from .distributed import log_evidence_from_sums
        tr = self._trainer
        self._check_mvn_family("posterior_grid")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        sums, out, box = tr._ctx.posterior_grid(x, m, p5, sg, q=q, **grid_kw)
        lead = data.shape[:-1]
        col = lambda i: out[:, i].reshape(lead)   # noqa: E731
        lp, el, gap = log_evidence_from_sums(sums)
        return dict(log_evidence=col(0), elbo=col(1), gap=col(0) - col(1), oef=col(2), dbv=col(3), r2p=col(4),
                    oef_sd=col(5), dbv_sd=col(6), r2p_sd=col(7), corr=col(8),
                    oef_ci=out[:, 9:11].reshape(lead + (2,)), dbv_ci=out[:, 11:13].reshape(lead + (2,)),
                    map=out[:, 13:15].reshape(lead + (2,)), edge_mass=col(15), quad_err=col(16),
                    box=None if box is None else box.reshape(lead + (4,)), sums=sums, mean_log_evidence=lp,
                    mean_elbo=el, mean_gap=gap)

    def laplace(self, data, mask, prior, start="prior", **cfg):
        """Per-voxel Laplace posteriors on any tau grid (Context.laplace_posterior; cfg: max_iter, tol, lambda0,
        lambda_up, lambda_down): the MAP of the log-joint by Levenberg-Marquardt -- the classical non-linear
        least-squares fit under the prior -- and the Gauss-Newton curvature there, with the sigma refine() takes (the
        encoder's sigma head or the fine tuner's homoscedastic sigma).  start = "prior": from the prior mean;
        "encoder": from the encoder heads' means.  Shaped like the data's spatial dims:
          q [..., 5] (raw heads of N(u^, A^-1): goes unchanged to calculate_means, elbo(q=...), log_evidence(q=...),
            posterior_grid(q=...), posterior_predictive(q=...), loo, calibration), map [..., 2] (logits a^, b^)
          oef, dbv, r2p at the MAP and oef_sd, dbv_sd, r2p_sd (delta method), logit_sd [..., 2], corr
          log_evidence (Laplace), chi2, iterations, converged, on_clip, clamped (bool; clamped: the heads could not
            hold the covariance exactly)
        Voxels outside the mask are NaN (False in the flags) and keep the prior's row in q."""
        tr = self._trainer
        self._check_mvn_family("laplace")
        if start not in ("prior", "encoder"):
            raise ValueError("laplace: start must be 'prior' or 'encoder'")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data)
        u0 = q[:, [0, 2]].contiguous() if start == "encoder" else None
        q_out, out = tr._ctx.laplace_posterior(x, m, p5, sg, u0=u0, **cfg)
        lead = data.shape[:-1]
        col = lambda i: out[:, i].reshape(lead)   # noqa: E731
        flags = torch.nan_to_num(out[:, 14], nan=0.0).to(torch.int32)
        live = ~torch.isnan(out[:, 14])
        bit = lambda b: (((flags >> b) & 1) == 1).reshape(lead)   # noqa: E731
        return dict(q=q_out.reshape(lead + (5,)), map=out[:, 0:2].reshape(lead + (2,)), oef=col(2), dbv=col(3),
                    r2p=col(4), logit_sd=out[:, 5:7].reshape(lead + (2,)), corr=col(7), oef_sd=col(8), dbv_sd=col(9),
                    r2p_sd=col(10), log_evidence=col(11), chi2=col(12), iterations=col(13),
                    converged=(live & ((flags & 1) == 0)).reshape(lead), on_clip=bit(1), clamped=bit(2))

    def identifiability(self, data, mask, prior, q=None, no_samples=200):
        """How well the protocol can determine OEF and DBV in each voxel at all (Context.fisher_information): the Fisher
        information of the fitted likelihood -- independent noise sigma on the normalised data, the normaliser's own
        noise ignored -- at the posterior means of the heads q [..., 5] (None: the encoder's), with the sigma refine()
        takes.  A wide posterior beside a wide bound is the protocol's doing, beside a narrow one the encoder's.
        Shaped like the data's spatial dims:
          oef_crlb, dbv_crlb, r2p_crlb (data-only Cramer-Rao sds), corr, kappa (correlation and conditioning of the data
            information: the OEF . DBV ridge), singular (bool)
          oef_bound, dbv_bound, r2p_bound (sds from (I + Lambda)^-1, Lambda the prior's precision)
          oef_ratio, dbv_ratio, r2p_ratio: the posterior sd (calculate_means(return_stds=True), `no_samples` draws) over
            its Bayesian bound
        Voxels outside the mask are NaN."""
        tr = self._trainer
        self._check_mvn_family("identifiability")
        T = data.shape[-1]
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        means, var = tr.calculate_means(q, None, include_r2p=True, return_stds=True, no_samples=no_samples)
        f = tr._ctx.fisher_information(means[:, :2].contiguous(), sg.reshape(-1, T), None, p5, m)
        lead = data.shape[:-1]
        out = {k: f[k].reshape(lead) for k in ("oef_crlb", "dbv_crlb", "r2p_crlb", "corr", "kappa", "singular",
                                                "oef_bound", "dbv_bound", "r2p_bound")}
        sd = torch.sqrt(var)
        for i, k in enumerate(("oef", "dbv", "r2p")):
            out[k + "_ratio"] = (sd[:, i] / f[k + "_bound"]).reshape(lead)
        return out

    def adapt(self, data, mask, prior, q=None, rounds=6, no_samples=64, shrink=4.0, seed=1, voxel0=0):
        """Adaptive importance sampling per voxel by moment matching (Context.adapt_posterior; Paananen et al. 2021):
        `rounds` rounds of `no_samples` draws, after each of which the proposal moves to the importance-weighted mean
        and covariance of its own draws (the mass-covering forward-KL projection, shrunk by ESS / (ESS + shrink)) --
        the remedy for voxels whose log_evidence(psis=True) k^ says the importance estimates cannot be trusted.  Starts
        from the encoder heads of encoder_model.predict, from given heads q [..., 5] (laplace()'s or refine()'s), or,
        q = "prior", from the prior itself (no encoder heads involved, as laplace(start="prior")); sigma as refine()
        takes it.  Shaped like the data's spatial dims:
          q [..., 5] (raw heads of the round with the largest ESS: goes unchanged to calculate_means, elbo(q=...),
            log_evidence(q=..., psis=True), posterior_grid(q=...), posterior_predictive(q=...), loo, calibration)
          log_evidence, ess [..., rounds] (each round's log p^ and ESS of no_samples), best (the returned round),
          flags (int32: 1 a round skipped for non-finite weights, 2 a mean on the logit clip, 4 a spread head clamped)
        Voxels outside the mask keep their starting heads and are NaN (best -1, flags 0)."""
        tr = self._trainer
        self._check_mvn_family("adapt")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        if isinstance(q, str):
            if q != "prior":
                raise ValueError("adapt: q must be heads [..., 5], None (the encoder's) or 'prior'")
            _, sg = self._heads_and_sigma(data)
            q0 = p5
        else:
            q0, sg = self._heads_and_sigma(data, q)
        q_out, out = tr._ctx.adapt_posterior(x, m, q0, p5, sg, rounds=rounds, K=no_samples, shrink=shrink, seed=seed,
                                             voxel0=voxel0)
        lead = data.shape[:-1]
        R = (out.shape[1] - 2) // 2
        live = ~torch.isnan(out[:, 2 * R])
        best = torch.where(live, torch.nan_to_num(out[:, 2 * R], nan=0.0).to(torch.int32),
                           torch.full_like(out[:, 0], -1, dtype=torch.int32))
        flags = torch.nan_to_num(out[:, 2 * R + 1], nan=0.0).to(torch.int32)
        return dict(q=q_out.reshape(lead + (5,)), log_evidence=out[:, 0:2 * R:2].reshape(lead + (R,)),
                    ess=out[:, 1:2 * R:2].reshape(lead + (R,)), best=best.reshape(lead), flags=flags.reshape(lead))

    def posterior_predictive(self, data, mask, q=None, no_samples=256, seed=1, voxel0=0, want_curves=False):
        """Posterior predictive checks of `no_samples` = L draws per voxel (Context.posterior_predictive) for the heads q
        [..., 5] (None: the encoder heads of encoder_model.predict; refine()'s output, say) and the sigma that goes with
        them, in the likelihood's own space.  Shaped like the data's spatial dims:
          ppp        posterior predictive p-value of the chi2 discrepancy (small: the model misfits the voxel; NaN under
                     Student-t)
          dbar       mean chi2 discrepancy;  lppd, p_waic, elpd_waic = lppd - p_waic (pointwise predictive accuracy)
          max_abs_z  the largest standardised residual over the taus
          pred_mean, pred_sd, std_resid [..., T] (want_curves): the fitted curve, its predictive sd, (y - mean) / sd
        and the masked sums with mean_elpd_waic, mean_p_waic, mean_ppp (distributed.ppc_from_sums).  Voxels outside
        the mask are NaN."""
        from .distributed import ppc_from_sums
        tr = self._trainer
        self._check_mvn_family("posterior_predictive")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        q, sg = self._heads_and_sigma(data, q)
        sums, out, curves = tr._ctx.posterior_predictive(x, m, q, sg, L=no_samples, seed=seed, voxel0=voxel0,
                                                         want_curves=want_curves)
        lead = data.shape[:-1]
        res = {k: out[:, i].reshape(lead) for i, k in enumerate(tr._ctx.PPC_COLUMNS)}
        if curves is not None:
            res.update(pred_mean=curves[..., 0].reshape(lead + (T,)), pred_sd=curves[..., 1].reshape(lead + (T,)),
                       std_resid=curves[..., 2].reshape(lead + (T,)))
        el, pw, pp = ppc_from_sums(sums)
        res.update(sums=sums, mean_elpd_waic=el, mean_p_waic=pw, mean_ppp=pp)
        return res


    def loo(self, data, mask, prior, q=None, no_samples=256, seed=1, voxel0=0, want_pointwise=False):
        """PSIS leave-one-out cross-validation per voxel and per tau image (Context.loo; Vehtari, Gelman & Gabry 2017)
        of `no_samples` = K draws (25 <= K <= 1024, the draws of log_evidence() for the same seed) for the heads q
        [..., 5] (None: the encoder heads of encoder_model.predict; refine()'s output, say) and the sigma that goes with
        them.  Shaped like the data's spatial dims:
          elpd_loo   sum_t log p(y_t | y_-t): compares forward-model variants on the same data
          p_loo      lppd - elpd_loo, the effective number of parameters;  lppd from the smoothed full-data weights
          khat_max   the largest Pareto k^ over the tau images (above 0.7: elpd_loo is not reliable there, and ONE image
                     dominates the voxel's fit -- the signature of a corrupted tau image), worst_tau its index
          khat_full  the k^ of the full-data weights (log_evidence(psis=True)'s khat)
          elpd_t, khat_t, lppd_t [..., T] (want_pointwise)
        and the masked sums with mean_elpd_loo, mean_p_loo, frac_khat_bad (distributed.loo_from_sums).  Voxels outside
        the mask are NaN."""
        from .distributed import loo_from_sums
        tr = self._trainer
        self._check_mvn_family("loo")
        T = data.shape[-1]
        x = _flat(data, T)
        m = None if mask is None else mask.reshape(-1)
        p5 = _flat(prior, prior.shape[-1]).contiguous()
        q, sg = self._heads_and_sigma(data, q)
        r = tr._ctx.loo(x, m, q, p5, sg, int(no_samples), seed=seed, voxel0=voxel0, want_pointwise=want_pointwise)
        lead = data.shape[:-1]
        res = {k: r["out"][:, i].reshape(lead) for i, k in enumerate(tr._ctx.LOO_COLUMNS)}
        if want_pointwise:
            pw = r["pointwise"]
            res.update(elpd_t=pw[..., 0].reshape(lead + (T,)), khat_t=pw[..., 1].reshape(lead + (T,)),
                       lppd_t=pw[..., 2].reshape(lead + (T,)))
        el, pl, bad = loo_from_sums(r["sums"])
        res.update(sums=r["sums"], mean_elpd_loo=el, mean_p_loo=pl, frac_khat_bad=bad)
        return res


class EncoderTrainer:
    def __init__(self,
                 system_params,
                 no_intermediate_layers=1,
                 no_units=10,
                 use_layer_norm=False,
                 dropout_rate=0.0,
                 activation_type='gelu',
                 student_t_df=None,
                 initial_im_sigma=0.08,
                 multi_image_normalisation=True,
                 channelwise_gating=False,
                 infer_inv_gamma=False,
                 use_mvg=True,
                 use_population_prior=True,
                 mog_components=1,
                 no_samples=1,
                 heteroscedastic_noise=True,
                 predict_log_data=True,
                 full_model=True,
                 use_blood=True,
                 device=None,
                 seed=1):
        self._no_intermediate_layers = no_intermediate_layers
        self._no_units = no_units
        self._use_layer_norm = use_layer_norm
        self._dropout_rate = dropout_rate
        self._activation_type = activation_type
        self._student_t_df = student_t_df
        self._initial_im_sigma = initial_im_sigma
        self._multi_image_normalisation = multi_image_normalisation
        self._system_params = system_params
        self._channelwise_gating = channelwise_gating
        self._infer_inv_gamma = infer_inv_gamma
        self._use_mvg = use_mvg
        self._nq = 5 if use_mvg else 4   # parameters of the predicted distribution (model.py:191-193)
        self._use_population_prior = use_population_prior
        self._mog_components = mog_components
        self._no_samples = no_samples
        self._kl_tiled = True   # KL draws per voxel = no_samples x kl_samples, as the reference's tiled batch gives
        self._oef_range = 0.8
        self._min_oef = 0.04
        self._dbv_range = 0.2
        self._min_dbv = 0.001
        self._heteroscedastic_noise = heteroscedastic_noise
        self._predict_log_data = predict_log_data
        self._full_model = full_model
        self._use_blood = use_blood
        # Store the spin-echo index (model.py:95)
        self._se_idx = int(abs(float(system_params['tau_start']) / float(system_params['tau_step'])))
        self._seed = int(seed)
        unsupported = []
        if activation_type not in ('relu', 'gelu'):
            unsupported.append(f"activation_type={activation_type!r} (kernels implement 'relu' and 'gelu')")
        if infer_inv_gamma and use_mvg:
            # the reference itself cannot run this pair: synthetic_data_loss splits the 9-channel first output
            # (5 + 4) in two (tf.split(y_pred_orig, 2, axis=-1), model.py:455)
            unsupported.append("infer_inv_gamma with use_mvg=True (a shape error in the reference, model.py:455; "
                               "the learned hyper-prior runs with the diagonal family, use_mvg=False)")
        if use_population_prior and use_mvg:
            # the reference cannot run this pair either: kl_loss hands the 10-channel 'predictions' to
            # logit_gaussian_mvg_log_prob, which reshapes them to (-1, 5) and so doubles the rows (model.py:596, 378)
            unsupported.append("use_population_prior with use_mvg=True (a shape error in the reference, model.py:596; "
                               "the population prior runs with the diagonal family, use_mvg=False)")
        if use_population_prior and not use_mvg and mog_components > 16:
            unsupported.append("mog_components > 16")
        if unsupported:
            raise NotImplementedError("configuration outside the accelerated path (disabled by "
                                      "configurations/optimal.yaml): " + "; ".join(unsupported))
        self._ctx = Context(system_params, full_model, use_blood,
                            multi_image_normalisation=multi_image_normalisation,
                            predict_log_data=predict_log_data, student_t_df=student_t_df,
                            device=device)
        assert self._ctx.se_idx == self._se_idx

    # ------------------------------------------------------------------------------------
    @property
    def context(self):
        return self._ctx

    @staticmethod
    def _is_spatial(x):
        return x.dim() == 5 and (x.shape[1] > 1 or x.shape[2] > 1)

    def _spatial_state(self, weights):
        from .ops import TrainState
        st = getattr(weights, "_spatial_state", None)
        if st is None:
            if weights.shape.spatial_taps != 9:
                raise ValueError("image crops need an encoder created with 3x3x1 kernels (spatial_taps=9)")
            st = weights._spatial_state = TrainState(self._ctx, weights, optimiser_state=False)
        return st

    def normalise_data(self, _data):  # model.py:97-113
        return self._ctx.normalise(_data)

    def create_encoder(self, system_constants=None, gate_offset=0.0, resid_init_std=1e-1,
                       no_ip_images=11):
        """model.py:122-223.  Returns (outer_model, inner_model)."""
        if no_ip_images != self._ctx.T:
            raise ValueError("no_ip_images must equal the number of taus of the system parameters")
        # the residual stream owns full 3x3x1 kernels as in the reference (146,176 parameters at
        # optimal.yaml); voxel batches act through their centre tap
        w = init_encoder_weights(T=no_ip_images, U=self._no_units, L=self._no_intermediate_layers,
                                 channelwise_gating=self._channelwise_gating,
                                 resid_init_std=resid_init_std, im_loss_sigma=self._initial_im_sigma,
                                 seed=self._seed, spatial_taps=9, layer_norm=self._use_layer_norm)
        if not self._use_mvg:  # 4 outputs: the Cholesky column of the 5-wide head stays exactly zero
            w["Wf"][:, 4] = 0.0
            w["bf"][4] = 0.0
        ew = EncoderWeights(self._ctx, no_ip_images, self._no_units, self._no_intermediate_layers,
                            self._channelwise_gating, gate_offset, spatial_taps=9,
                            activation=self._activation_type, layer_norm=self._use_layer_norm,
                            dropout_rate=self._dropout_rate).set_from_arrays(w)
        return EncoderModel(self, ew), _InnerModel()

    def build_fine_tuner(self, encoder_model, signal_generation_layer, input_im=None, input_mask=None):
        return FineTuner(self, encoder_model, signal_generation_layer)  # model.py:239-286

    # -- transforms (model.py:288-316) -----------------------------------------------------
    def transform_std(self, pred_stds):
        return self._ctx.transform("transform_std", pred_stds)

    def transform_offdiag(self, pred_offdiag):
        return self._ctx.transform("transform_offdiag", pred_offdiag)

    def inv_transform_std(self, std):
        return self._ctx.transform("inv_transform_std", std)

    def forward_transform(self, logits):
        return self._ctx.transform("forward_transform", logits)

    def backwards_transform(self, signal, include_logit):
        return self._ctx.transform("backwards_transform_logit" if include_logit
                                   else "backwards_transform", signal)

    # -- sampling / moments (model.py:318-374) -----------------------------------------------
    def kl_draws(self, kl_samples, no_samples=None, kl_tiled=None):
        """KL draws per voxel: kl_samples per copy of the S-fold tiled batch of the reference (model.py:245-246, 656),
        i.e. S * kl_samples, unless kl_tiled is off."""
        S = self._no_samples if no_samples is None else no_samples
        tiled = self._kl_tiled if kl_tiled is None else kl_tiled
        return int(kl_samples) * (int(S) if tiled else 1)

    def create_samples(self, predicted_params, mask, no_samples, seed=None):
        q = _pad5(_flat(predicted_params, predicted_params.shape[-1])[:, :self._nq]).contiguous()
        z = self._ctx.normals(q.shape[0], no_samples, stream_id=2,
                              seed=self._seed if seed is None else seed)
        qs = q[:, None, :].expand(-1, no_samples, -1).reshape(-1, 5)
        s = self._ctx.reparam(qs, z.reshape(-1, 2)).reshape(q.shape[0], no_samples, 2)
        return s.permute(0, 2, 1).reshape(predicted_params.shape[:-1] + (2, no_samples))

    def calculate_means(self, predicted_params, mask, include_r2p=False, return_stds=False,
                        no_samples=20, seed=None):
        q = _pad5(_flat(predicted_params, predicted_params.shape[-1])[:, :self._nq]).contiguous()
        means, var = self._ctx.posterior_moments(q, no_samples, seed=self._seed if seed is None else seed,
                                                 want_vars=return_stds)
        c = 3 if include_r2p else 2
        lead = predicted_params.shape[:-1]
        means = means[:, :c].reshape(lead + (c,))
        if return_stds:  # NB: biased variances under the name "stds" (model.py:331, Appendix B9)
            return means, var[:, :c].reshape(lead + (c,))
        return means

    def calibration(self, model, n_voxels=65536, no_samples=255, seed=1, fine_tuner=None, prior=None, psis=False,
                    use_first_op=False, uniform_prop=0.0, bins=16):
        """Do the encoder's posteriors cover as often as they claim?  Simulates n_voxels voxels with known (OEF, DBV)
        (training.synthetic_voxel_dataset: the pre-training priors, forward model and noise), takes the heads of stream 1
        (use_first_op) or stream 2 and places each truth in its posterior (Context.calibration, `no_samples` draws per
        voxel).  Returns FineTuner.calibration's dict(out [N, 6], khat, summary); the summary gains z_mean and z_rms of
        (OEF, DBV, R2'): (posterior mean - truth) / posterior sd from Context.posterior_moments at `no_samples` draws,
        0 and 1 for a calibrated posterior.
        fine_tuner: score that fine tuner's model (its sigma; psis=True with a [N, 5] `prior` ranks under the
        importance-corrected posterior); without one the heads go to Context.calibration directly."""
        from .calibration import summarise
        from .training import synthetic_voxel_dataset
        if not self._use_mvg:
            raise NotImplementedError("calibration works on the use_mvg=True family; the diagonal family draws with "
                                      "exp(raw_s), not transform_std (model.py:696-698)")
        if psis and fine_tuner is None:
            raise ValueError("calibration(psis=True) needs the fine_tuner whose likelihood the weights are taken under")
        cfg = dict(uniform_prop=uniform_prop, full_model=self._full_model, use_blood=self._use_blood)
        x, mask, y = synthetic_voxel_dataset(self._system_params, cfg, int(n_voxels), self._ctx.device, seed)
        o1, o2, _ = model.predict(x, want=("out1",) if use_first_op else ("out2",))
        q = _flat((o1 if use_first_op else o2)[..., :5], 5).contiguous()
        L = int(no_samples)
        if fine_tuner is not None:
            res = fine_tuner.calibration(x, y, mask, prior=prior, no_samples=L, q=q, psis=psis, seed=seed, bins=bins)
        else:
            out = self._ctx.calibration(y, q, mask, L=L, seed=seed)
            res = dict(out=out, khat=None, summary=summarise(out, L, bins=bins))
        means, var = self._ctx.posterior_moments(q, L, seed=seed)
        truth = torch.cat([y, self.calculate_r2p(y[:, :1], y[:, 1:2])], 1)
        zs = ((means - truth) / var.sqrt()).double()
        zs = zs[torch.isfinite(zs).all(1)]
        res["summary"]["z_mean"] = [float(v) for v in zs.mean(0)]
        res["summary"]["z_rms"] = [float(v) for v in (zs * zs).mean(0).sqrt()]
        return res

    def oef_dbv_metrics(self, y_true, y_pred, oef_dbv_r2p=0):
        means = self.calculate_means(y_pred, None, include_r2p=True)
        residual = (means.reshape(-1, 3) - y_true.reshape(-1, 3))[:, oef_dbv_r2p]
        return torch.mean(residual * residual)

    def oef_metric(self, y_true, y_pred):
        return self.oef_dbv_metrics(y_true, y_pred, 0)

    def dbv_metric(self, y_true, y_pred):
        return self.oef_dbv_metrics(y_true, y_pred, 1)

    def r2p_metric(self, y_true, y_pred):
        return self.oef_dbv_metrics(y_true, y_pred, 2)

    # -- log density (model.py:376-447) ------------------------------------------------------
    def logit_gaussian_mvg_log_prob(self, observations, predicted_params):
        shape = predicted_params.shape[:-1]
        out = self._ctx.logit_mvn_nlogp(observations.reshape(-1, observations.shape[-1])[:, 0:2],
                                        _flat(predicted_params, 5))
        return out.reshape(shape)

    @staticmethod
    def calculate_log_chol_det(oef_log_std, dbv_log_std):
        return 2.0 * (oef_log_std + dbv_log_std)

    @staticmethod
    def squared_whitened_residual(obs, mean, oef_log_std, dbv_log_std, oef_dbv_cov):   # model.py:423-441
        from .logit_mvn import LogitMVN
        return LogitMVN.squared_whitened_residual(obs, mean, oef_log_std, dbv_log_std, oef_dbv_cov)

    def logit_gaussian_log_prob(self, observations, predicted_params):
        """Diagonal family (model.py:406-421): the 5-parameter density with a zero Cholesky term, less
        the log 2 pi that the reference's gaussian_nll (:403-404) does not carry."""
        shape = predicted_params.shape[:-1]
        p = _pad5(_flat(predicted_params, predicted_params.shape[-1])[:, :4]).contiguous()
        out = self._ctx.logit_mvn_nlogp(observations.reshape(-1, observations.shape[-1])[:, 0:2], p)
        return (out - 1.8378770664093453).reshape(shape)

    def synthetic_data_loss(self, y_true_orig, y_pred_orig, use_r2p_loss=False, inv_gamma_alpha=0.0,
                            inv_gamma_beta=0.0):
        """Pre-training loss (model.py:449-514): mean negative log density of the true (OEF, DBV),
        plus the inverse-gamma prior on the marginal variances when alpha * beta > 0 (:492-507)."""
        y = y_true_orig.reshape(-1, 3).contiguous()
        hyper = None
        if self._infer_inv_gamma:   # y_pred = [4 parameters | 4 exp-activated hyper-parameters], model.py:454-455
            flat = _flat(y_pred_orig, y_pred_orig.shape[-1])
            if flat.shape[-1] != 8:
                raise ValueError("infer_inv_gamma: y_pred must carry 4 + 4 channels (model.py:201-205)")
            hyper = [float(v) for v in flat[0, 4:8].tolist()]   # inv_gamma_params[0,0,0,0,:], model.py:494
            y_pred_orig = flat[:, :4]
        q = _pad5(_flat(y_pred_orig, y_pred_orig.shape[-1])[:, :self._nq]).contiguous()
        offset = 0.0 if self._use_mvg else 1.8378770664093453   # logit_gaussian_log_prob, model.py:470
        if hyper is not None:   # model.py:493-498: with infer_inv_gamma the learned prior is the ONLY one
            inv_gamma_alpha = inv_gamma_beta = 0.0
        if inv_gamma_alpha * inv_gamma_beta > 0.0:
            lv = self._ctx.synth_loss(y, q, inv_gamma_alpha, inv_gamma_beta)
        else:
            lv = self._ctx.logit_mvn_nlogp(y[:, :2], q)
        if hyper is not None:   # - log IG(exp(2 s_o); a_o, b_o) - log IG(exp(2 s_d); a_d, b_d), model.py:495-507
            lv = lv.clone()
            self._ctx.hyper_prior_bwd(q, hyper, loss_v=lv, want_stats=False)
        if use_r2p_loss:   # model.py:475-490: ten reparameterised draws, a normal fitted to their R2'
            self._r2p_calls = getattr(self, "_r2p_calls", 0) + 1
            lv = lv.clone()
            self._ctx.r2p_loss_bwd(y, q, R2P_LOSS_SAMPLES, seed=self._r2p_calls, loss_v=lv, want_grad=False)
        return lv.mean() - offset

    def calculate_dw(self, oef):  # model.py:516-522
        from .signals import SignalGenerationLayer
        p = self._system_params
        return SignalGenerationLayer.calculate_dw_static(oef, float(p['hct']), float(p['gamma']),
                                                         float(p['b0']), float(p['dchi']))

    def calculate_r2p(self, oef, dbv):
        return self.calculate_dw(oef) * dbv

    # -- objective terms ---------------------------------------------------------------------
    def fine_tune_loss_fn(self, y_true, y_pred, return_mean=True):
        """model.py:527-568.  y_true [..., T+1] = [data, mask]; y_pred [S*..., 2T] = [signal, sigma], or
        [S*..., T+1] = [signal, one channel of the scalar sigma] with heteroscedastic_noise=False (:535-537)."""
        T = self._ctx.T
        yt = _flat(y_true, T + 1)
        yp = _flat(y_pred, 2 * T if self._heteroscedastic_noise else T + 1)
        S = self._no_samples
        N = yt.shape[0]
        if yp.shape[0] != N * S:
            raise ValueError("y_pred must hold no_samples copies of the batch")
        mask = yt[:, T].contiguous()
        if self._heteroscedastic_noise:
            sig = yp[:, T:]
        else:   # sigma = reduce_mean(y_pred[..., -1:]) (model.py:536): the mean of the constant channel
            sig = yp[:, T:].mean().expand(yp.shape[0], T).contiguous()
        nll = self._ctx.nll_fwd(yt[:, :T], mask, yp[:, :T], sig, S)
        nll = nll * mask.repeat(S)                       # model.py:564
        if return_mean:
            return nll.sum() / (mask.sum() * S)          # model.py:566 (mask is tiled S times)
        return nll.reshape((S * y_true.shape[0],) + tuple(y_true.shape[1:-1]) + (1,))

    def mvg_kl_samples(self, prior, pred, no_samples=50, seed=None):  # model.py:592-610
        pr = _flat(prior, 6)
        kl = self._ctx.kl_fwd(_flat(pred, 5), pr[:, :5], K=no_samples,
                              seed=self._seed if seed is None else seed)
        return kl.reshape(pred.shape[:-1] + (1,))

    def mvg_kl(self, true, predicted):  # model.py:612-652 (closed form; cross-check)
        pr = _flat(true, 6)
        return self._ctx.kl_closed(_flat(predicted, 5), pr[:, :5]).reshape(predicted.shape[:-1] + (1,))

    def kl_loss(self, true, predicted, return_mean=True, no_samples=70, seed=None):  # model.py:654-724
        true = torch.cat([true] * self._no_samples, 0)
        if not self._use_mvg:  # closed form per dimension, model.py:686-721
            pr = _flat(true, 5)   # [p_oef_mean, p_oef_log_std, p_dbv_mean, p_dbv_log_std, mask]
            pred = _flat(predicted, predicted.shape[-1])
            prior_cost = 0.0
            if self._use_population_prior and self._mog_components > 1:   # model.py:666-685
                M = int(self._mog_components)
                if pred.shape[-1] != 4 + 4 * M:
                    raise ValueError("mog_components: predictions must carry 4 + 4 M channels (model.py:262-270)")
                kl = self._ctx.kl_mog(_pad5(pred[:, :4]).contiguous(), pred[0, 4:].reshape(M, 4).contiguous(),
                                      seed=self._seed if seed is None else seed)
                kl_op = kl.reshape(predicted.shape[:-1] + (1,))
                mask = true[..., 4:5]
                kl_op = torch.where(mask > 0, kl_op, torch.zeros_like(kl_op))
                return kl_op.sum() / mask.sum() if return_mean else kl_op
            if self._use_population_prior:   # 'predictions' = [q4 | population prior 4]; `true` gives the mask only
                if pred.shape[-1] != 8:
                    raise ValueError("use_population_prior: predictions must carry 4 + 4 channels (model.py:268-270)")
                prior4 = pred[:, 4:8]
                prior_cost = self.population_prior_cost(prior4[0], predicted.shape[0])
            else:
                prior4 = pr[:, :4]
            _, kl = self._ctx.kl_diag(_pad5(pred[:, :4]).contiguous(), _pad5(prior4).contiguous())
            kl_op = kl.reshape(predicted.shape[:-1] + (1,))
            mask = true[..., 4:5]
            kl_op = torch.where(mask > 0, kl_op, torch.zeros_like(kl_op))
            return (kl_op.sum() + prior_cost) / mask.sum() if return_mean else kl_op
        kl_op = self.mvg_kl_samples(true, predicted, no_samples=no_samples, seed=seed)
        mask = true[..., 5:6]
        kl_op = torch.where(mask > 0, kl_op, torch.zeros_like(kl_op))
        if return_mean:
            return kl_op.sum() / mask.sum()
        return kl_op

    def population_prior_cost(self, prior4, batch):
        """model.py:710-716: -log IG(1, 2) of exp(2 * log-std) for the population prior's DBV and OEF log-stds (after
        transform_std), times the size of the batch axis (tf.shape(predicted)[0]).  Four scalars: host float64."""
        p = [float(v) for v in (prior4.tolist() if hasattr(prior4, "tolist") else prior4)]
        cost = 0.0
        for raw in (p[3], p[1]):
            log_std = 3.0 * math.tanh(raw) - 1.0
            v = math.exp(2.0 * log_std)
            cost -= math.log(2.0) - 2.0 * math.log(v) - 2.0 / v     # log IG(v; 1, 2)
        return cost * float(batch)

    def smoothness_loss(self, true_params, pred_params):
        """Total-variation term (model.py:726-754): sum of |differences| of the range-scaled
        forward-transformed means over x / y neighbours with both masks set, over sum(mask).
        Identically 0 for voxel batches."""
        true_params = torch.cat([true_params] * self._no_samples, 0)
        if not self._is_spatial(pred_params):
            return torch.zeros((), dtype=torch.float32, device=pred_params.device)
        mask = true_params[..., self._nq]   # model.py:729-734
        tv = self._ctx.smoothness(_pad5(pred_params[..., :self._nq]).contiguous(), mask)
        return (tv[0] / mask.sum()).float()

    def estimate_population_param_distribution(self, model, data):
        """model.py:756-770: masked population mean / std of the predicted OEF and DBV logits of the SECOND
        output (`_, predictions, _ = model.predict(...)`, model.py:757: the stream-2 / fine-tuned head, which
        sees the 3x3x1 context on volumes), printed and returned as (mean_oef, log_std_oef, mean_dbv,
        log_std_dbv)."""
        predictions = model.predict(data[..., :-1] * data[..., -1:], want=("out2",))[1]
        mask = data[..., -1:]
        oef, dbv = predictions[..., 0:1] * mask, predictions[..., 2:3] * mask
        mask_pix = mask.sum()
        out = []
        for v in (oef, dbv):
            mean = v.sum() / mask_pix
            std = torch.sqrt((torch.square(v - mean) * mask).sum() / mask_pix)
            out += [mean, self.inv_transform_std(torch.log(std).reshape(1))[0]]
        print('final results for mean_oef, log_std_oef, mean_dbv, log_std_dbv, respectively: ')
        print(*[float(o) for o in out])
        return tuple(out)

    def save_predictions(self, model, data, filename, transform_directory=None, use_first_op=True,
                         fine_tuner_model=None, priors=None, iw_samples=None, refine_steps=None,
                         posterior_grid=None, ppc_samples=None, refine_smoothness_weight=0.0, psis=False,
                         loo_samples=None, laplace=False, adapt_rounds=None, identifiability=False,
                         interval_samples=None):
        """model.py:772-887: write `<filename>_{oef,dbv,r2p,logstds}.nii.gz` (posterior means of
        OEF / DBV / R2' over 200 draws and their variances) and, with a fine tuner,
        `_likelihood` (per-voxel NLL averaged over 100 stochastic passes), `_kl` (100-draw KL to
        `priors`) and `_residual` (mean |normalised data - one sampled prediction|).
        iw_samples = K (with a fine tuner; this package's addition): also `_logevidence` (importance-weighted
        log p^ of K draws, FineTuner.log_evidence), `_vigap` (log p^ - the same draws' ELBO) and `_ess` (effective
        sample size), zero outside the mask; the three maps [subj, X, Y, Z, 1] are returned as a dict.
        psis = True (with iw_samples = K, 25 <= K <= 1024): Pareto-smoothed importance sampling of the same draws
        (FineTuner.log_evidence(psis=True)) as `_khat` (the tail shape k^ of the voxel's weights: the importance
        estimates are reliable below min(1 - 1 / log10 K, 0.7)), `_logevidence_psis`, `_ess_psis` and the smoothed-weight
        means `_oef_psis`, `_dbv_psis`, `_r2p_psis`, zero outside the mask; these maps join the returned dict.
        refine_steps (with a fine tuner; this package's addition): refine each voxel's heads by that many steps
        (FineTuner.refine) and also write `_oef_refined`, `_dbv_refined`, `_r2p_refined` (calculate_means of the
        refined heads) and `_amortgap` (per-voxel ELBO of the refined heads minus that of the encoder's, both from
        FineTuner.elbo(q=...) on the same draws; zero outside the mask); these maps join the returned dict.
        refine_smoothness_weight (with refine_steps): FineTuner.refine's smoothness_weight -- refine the volume under
        the TV prior of the fine-tuning loss too (5.0 in configurations/optimal.yaml); the maps keep their names.
        posterior_grid = True or a dict of grid keywords (with a fine tuner; this package's addition): the exact
        posterior by quadrature of the encoder's heads (FineTuner.posterior_grid) as `_oef_exact`, `_dbv_exact`,
        `_r2p_exact`, `_oef_exact_sd`, `_dbv_exact_sd`, `_oef_ci_lo`, `_oef_ci_hi`, `_dbv_ci_lo`, `_dbv_ci_hi`,
        `_logevidence_exact`, `_vigap_exact` (log p(x) - ELBO of the encoder's heads) and `_gridedge` (edge_mass),
        zero outside the mask; these maps join the returned dict.
        ppc_samples = L (with a fine tuner; this package's addition): posterior predictive checks of L draws from the
        encoder's heads (FineTuner.posterior_predictive) as `_ppp` (predictive p-value of the chi2 discrepancy),
        `_elpdwaic`, `_pwaic`, `_maxresid` (largest |standardised residual|) and the per-tau `_predmean`, `_predsd`,
        `_stdresid` [X, Y, Z, subj*T] (fitted curve, predictive sd, standardised residual in the likelihood's
        normalised space), zero outside the mask; these maps join the returned dict.  `_residual` is unchanged.
        loo_samples = K (with a fine tuner, 25 <= K <= 1024; this package's addition): PSIS leave-one-out
        cross-validation of K draws from the encoder's heads (FineTuner.loo) as `_elpdloo`, `_ploo`, `_khatloo` (the
        largest Pareto k^ over the tau images) and `_worsttau` (its tau index), NaN outside the mask; these maps join the
        returned dict.  None writes nothing new.
        laplace = True or a dict of FineTuner.laplace keywords (with a fine tuner; this package's addition, default
        off): the per-voxel Laplace posterior (Levenberg-Marquardt MAP fit under the prior, any tau grid) as
        `_oef_laplace`, `_dbv_laplace`, `_r2p_laplace`, `_oefsd_laplace`, `_dbvsd_laplace`, `_logevidence_laplace`,
        `_chi2` and `_laplaceflags` (bit 0 not converged, bit 1 on the logit clip, bit 2 heads clamped), zero outside
        the mask; these maps join the returned dict.
        adapt_rounds = R (with a fine tuner; this package's addition, default None writes nothing new): R rounds of
        adaptive importance sampling from the encoder's heads (FineTuner.adapt, 64 draws per round) as `_oef_adapt`,
        `_dbv_adapt`, `_r2p_adapt` (calculate_means of the adapted heads) and `_ess_adapt` (the returned round's ESS
        over its draws, in (0, 1]), zero outside the mask; with iw_samples (and psis) the importance maps above are
        taken under the adapted heads, so `_khat` is theirs.  These maps join the returned dict.
        identifiability = True (with a fine tuner; this package's addition, default off): what the protocol can
        determine at the encoder's posterior means (FineTuner.identifiability) as `_oef_crlb`, `_dbv_crlb`, `_r2p_crlb`
        (data-only Cramer-Rao sds), `_crlbcorr` and `_crlbkappa` (correlation and conditioning of the data information),
        zero outside the mask; these maps join the returned dict.
        interval_samples = K (with a fine tuner, 25 <= K <= 1024; this package's addition, default None writes nothing
        new): credible intervals of the importance-corrected posterior from K draws under their Pareto-smoothed weights
        (FineTuner.credible_intervals; the adapted heads when adapt_rounds is given) as `_oef_is_lo`, `_oef_is_hi`,
        `_dbv_is_lo`, `_dbv_is_hi`, `_r2p_is_lo`, `_r2p_is_hi` (the 2.5 % and 97.5 % weighted quantiles), `_oef_is_sd`,
        `_dbv_is_sd`, `_r2p_is_sd` and `_oefdbv_is_corr` (0 where an sd is 0: one effective draw), zero outside the
        mask; these maps join the returned dict.
        data [subj, X, Y, Z, T+1] with the mask last; each map is stored as [X, Y, Z, subj*C].
        `transform_directory/example.nii.gz`, when present, donates its header (:794-797); the
        FSL `applywarp`/`fslmerge` MNI step (:850-879) is preprocessing outside this package and
        is skipped."""
        import os
        from . import nifti
        if laplace and not fine_tuner_model:
            raise ValueError("save_predictions(laplace=True) needs a fine tuner (its sigma and the prior maps)")
        if adapt_rounds and not fine_tuner_model:
            raise ValueError("save_predictions(adapt_rounds=R) needs a fine tuner (its sigma and the prior maps)")
        if identifiability and not fine_tuner_model:
            raise ValueError("save_predictions(identifiability=True) needs a fine tuner (its sigma and the prior maps)")
        if interval_samples and not fine_tuner_model:
            raise ValueError("save_predictions(interval_samples=K) needs a fine tuner (its sigma and the prior maps)")
        data = torch.as_tensor(data, dtype=torch.float32, device=self._ctx.device)
        T = self._ctx.T
        mask = data[..., -1:]
        predictions, predictions2, _ = model.predict(data[..., :-1] * mask)
        if use_first_op is False:
            predictions = predictions2
        means, log_stds = self.calculate_means(predictions, torch.ones_like(predictions[..., :1]),
                                               include_r2p=True, return_stds=True, no_samples=200)
        template = None
        if transform_directory is not None:
            ex = os.path.join(transform_directory, 'example.nii.gz')
            if os.path.isfile(ex):
                template = nifti.load(ex)[1]

        def save_im_data(im_data, _filename):
            im = im_data.detach().cpu().numpy() if torch.is_tensor(im_data) else np.asarray(im_data)
            images = np.concatenate(np.split(im, im.shape[0], axis=0), axis=-1)[0]
            nifti.save(images.astype(np.float32), _filename + '.nii.gz', template)

        if fine_tuner_model:
            if priors is None:
                raise ValueError("save_predictions with a fine tuner needs the prior maps (train.py:272-279)")
            no_passes = 100
            out = fine_tuner_model.elbo(data[..., :-1], mask, torch.as_tensor(priors, device=data.device)[..., :self._nq],
                                        no_samples=no_passes * self._no_samples, kl_samples=100,
                                        seed=self._seed + 17)
            m = mask.reshape(-1)
            lik = (out["nll_kl"][:, 0] * m).reshape(data.shape[:4] + (1,))
            kl = torch.where(m > 0, out["nll_kl"][:, 1], torch.zeros_like(m)).reshape(data.shape[:4] + (1,))
            save_im_data(lik, filename + '_likelihood')
            save_im_data(kl, filename + '_kl')
            y_true = data[..., :-1]
            y_pred = fine_tuner_model.predict([y_true, mask])['predicted_images'][:data.shape[0], ..., :T]
            if self._multi_image_normalisation:
                sl = slice(self._se_idx - 1, self._se_idx + 2)
            else:
                sl = slice(self._se_idx, self._se_idx + 1)
            y_true = y_true / (y_true[..., sl].mean(-1, keepdim=True) + 1e-3)
            y_pred = y_pred / (y_pred[..., sl].mean(-1, keepdim=True) + 1e-3)
            save_im_data((y_true - y_pred).abs().mean(-1, keepdim=True), filename + '_residual')

        iw_maps = None
        q_adapt = ad_maps = None
        if fine_tuner_model and adapt_rounds:
            K_ad = 64   # draws per round
            ad = fine_tuner_model.adapt(data[..., :-1], mask, torch.as_tensor(priors, device=data.device)[..., :self._nq],
                                        rounds=int(adapt_rounds), no_samples=K_ad, seed=self._seed + 61)
            q_adapt = ad["q"]
            live = mask[..., 0] > 0
            ess = torch.gather(torch.nan_to_num(ad["ess"]), -1, ad["best"].clamp(min=0).long()[..., None])[..., 0] / K_ad
            a_means = self.calculate_means(q_adapt, None, include_r2p=True, no_samples=200)
            a_means = torch.where(live[..., None], a_means, torch.zeros_like(a_means))
            zero = torch.zeros_like(ess)
            ad_maps = {"oef_adapt": a_means[..., 0:1], "dbv_adapt": a_means[..., 1:2], "r2p_adapt": a_means[..., 2:3],
                       "ess_adapt": torch.where(live, ess, zero)[..., None]}
            for k, v in ad_maps.items():
                save_im_data(v, filename + '_' + k)
        if psis and not (fine_tuner_model and iw_samples):
            raise ValueError("save_predictions(psis=True) smooths the draws of iw_samples: give a fine tuner and iw_samples")
        if fine_tuner_model and iw_samples:
            iw = fine_tuner_model.log_evidence(data[..., :-1], mask,
                                               torch.as_tensor(priors, device=data.device)[..., :self._nq],
                                               no_samples=int(iw_samples), seed=self._seed + 31, psis=bool(psis),
                                               q=q_adapt)
            live = mask[..., 0] > 0
            zero = torch.zeros_like(iw["log_evidence"])
            iw_maps = {k: torch.where(live, v, zero)[..., None] for k, v in
                       (("logevidence", iw["log_evidence"]), ("vigap", iw["log_evidence"] - iw["elbo"]),
                        ("ess", iw["ess"]))}
            if psis:
                iw_maps.update({k: torch.where(live, v, zero)[..., None] for k, v in
                                (("khat", iw["khat"]), ("logevidence_psis", iw["log_evidence_psis"]),
                                 ("ess_psis", iw["ess_psis"]), ("oef_psis", iw["psis_means"][..., 0]),
                                 ("dbv_psis", iw["psis_means"][..., 1]), ("r2p_psis", iw["psis_means"][..., 2]))})
            for k, v in iw_maps.items():
                save_im_data(v, filename + '_' + k)
        if ad_maps:
            iw_maps = dict(ad_maps, **(iw_maps or {}))

        if fine_tuner_model and interval_samples:
            ci = fine_tuner_model.credible_intervals(data[..., :-1], mask,
                                                     torch.as_tensor(priors, device=data.device)[..., :self._nq],
                                                     q=q_adapt, no_samples=int(interval_samples), psis=True,
                                                     probs=(0.025, 0.975), seed=self._seed + 67)
            live = mask[..., 0] > 0
            zero = torch.zeros_like(ci["ess"])
            ci_maps = {}
            for i, name in enumerate(("oef", "dbv", "r2p")):
                ci_maps[name + "_is_lo"] = ci["quantiles"][..., i, 0]
                ci_maps[name + "_is_hi"] = ci["quantiles"][..., i, 1]
                ci_maps[name + "_is_sd"] = ci["sd"][..., i]
            ci_maps["oefdbv_is_corr"] = torch.nan_to_num(ci["corr_oef_dbv"], nan=0.0)   # undefined where an sd is 0
            ci_maps = {k: torch.where(live, v, zero)[..., None] for k, v in ci_maps.items()}
            for k, v in ci_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **ci_maps)

        if fine_tuner_model and refine_steps:
            x_ft = data[..., :-1]
            p_ft = torch.as_tensor(priors, device=data.device)[..., :self._nq]
            ref = fine_tuner_model.refine(x_ft, mask, p_ft, steps=int(refine_steps), seed=self._seed + 43,
                                          smoothness_weight=refine_smoothness_weight)
            q0, _ = fine_tuner_model._heads_and_sigma(x_ft)
            lead = data.shape[:4]

            def elbo_v(qq):   # per-voxel ELBO = -(nll + kl), the same seed (so the same draws) for both heads
                e = fine_tuner_model.elbo(x_ft, mask, p_ft, no_samples=32, kl_samples=70, seed=self._seed + 47,
                                          kl_tiled=False, q=qq)
                return -(e["nll_kl"][:, 0] + e["nll_kl"][:, 1])
            live = mask.reshape(-1) > 0
            gap = elbo_v(ref["q"].reshape(-1, 5)) - elbo_v(q0)
            gap = torch.where(live, gap, torch.zeros_like(gap))
            r_means = self.calculate_means(ref["q"], None, include_r2p=True, no_samples=200)
            ref_maps = {"oef_refined": r_means[..., 0:1], "dbv_refined": r_means[..., 1:2],
                        "r2p_refined": r_means[..., 2:3], "amortgap": gap.reshape(lead + (1,))}
            for k, v in ref_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **ref_maps)

        if fine_tuner_model and posterior_grid:
            kw = dict(posterior_grid) if isinstance(posterior_grid, dict) else {}
            pg = fine_tuner_model.posterior_grid(data[..., :-1], mask,
                                                 torch.as_tensor(priors, device=data.device)[..., :self._nq], **kw)
            live = mask[..., 0] > 0
            zero = torch.zeros_like(pg["oef"])
            grid_maps = {k: torch.where(live, v, zero)[..., None] for k, v in
                         (("oef_exact", pg["oef"]), ("dbv_exact", pg["dbv"]), ("r2p_exact", pg["r2p"]),
                          ("oef_exact_sd", pg["oef_sd"]), ("dbv_exact_sd", pg["dbv_sd"]),
                          ("oef_ci_lo", pg["oef_ci"][..., 0]), ("oef_ci_hi", pg["oef_ci"][..., 1]),
                          ("dbv_ci_lo", pg["dbv_ci"][..., 0]), ("dbv_ci_hi", pg["dbv_ci"][..., 1]),
                          ("logevidence_exact", pg["log_evidence"]), ("vigap_exact", pg["gap"]),
                          ("gridedge", pg["edge_mass"]))}
            for k, v in grid_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **grid_maps)

        if fine_tuner_model and ppc_samples:
            pc = fine_tuner_model.posterior_predictive(data[..., :-1], mask, no_samples=int(ppc_samples),
                                                       seed=self._seed + 53, want_curves=True)
            live = mask[..., 0] > 0
            zero = torch.zeros_like(pc["ppp"])
            ppc_maps = {k: torch.where(live, v, zero)[..., None] for k, v in
                        (("ppp", pc["ppp"]), ("elpdwaic", pc["elpd_waic"]), ("pwaic", pc["p_waic"]),
                         ("maxresid", pc["max_abs_z"]))}
            zt = torch.zeros_like(pc["pred_mean"])
            ppc_maps.update({k: torch.where(live[..., None], pc[c], zt) for k, c in
                             (("predmean", "pred_mean"), ("predsd", "pred_sd"), ("stdresid", "std_resid"))})
            for k, v in ppc_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **ppc_maps)

        if fine_tuner_model and loo_samples:
            lo = fine_tuner_model.loo(data[..., :-1], mask, torch.as_tensor(priors, device=data.device)[..., :self._nq],
                                      no_samples=int(loo_samples), seed=self._seed + 59)
            loo_maps = {k: lo[c][..., None] for k, c in (("elpdloo", "elpd_loo"), ("ploo", "p_loo"),
                                                         ("khatloo", "khat_max"), ("worsttau", "worst_tau"))}
            for k, v in loo_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **loo_maps)

        if fine_tuner_model and laplace:
            kw = dict(laplace) if isinstance(laplace, dict) else {}
            lp = fine_tuner_model.laplace(data[..., :-1], mask,
                                          torch.as_tensor(priors, device=data.device)[..., :self._nq], **kw)
            live = mask[..., 0] > 0
            zero = torch.zeros_like(lp["oef"])
            flags = (~lp["converged"]).float() + 2.0 * lp["on_clip"].float() + 4.0 * lp["clamped"].float()
            lap_maps = {k: torch.where(live, v, zero)[..., None] for k, v in
                        (("oef_laplace", lp["oef"]), ("dbv_laplace", lp["dbv"]), ("r2p_laplace", lp["r2p"]),
                         ("oefsd_laplace", lp["oef_sd"]), ("dbvsd_laplace", lp["dbv_sd"]),
                         ("logevidence_laplace", lp["log_evidence"]), ("chi2", lp["chi2"]), ("laplaceflags", flags))}
            for k, v in lap_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **lap_maps)

        if fine_tuner_model and identifiability:
            idf = fine_tuner_model.identifiability(data[..., :-1], mask,
                                                   torch.as_tensor(priors, device=data.device)[..., :self._nq])
            live = mask[..., 0] > 0
            id_maps = {k: torch.where(live, idf[src], torch.zeros_like(idf[src]))[..., None] for k, src in
                       (("oef_crlb", "oef_crlb"), ("dbv_crlb", "dbv_crlb"), ("r2p_crlb", "r2p_crlb"),
                        ("crlbcorr", "corr"), ("crlbkappa", "kappa"))}
            for k, v in id_maps.items():
                save_im_data(v, filename + '_' + k)
            iw_maps = dict(iw_maps or {}, **id_maps)

        save_im_data(means[..., 0:1], filename + '_oef')
        save_im_data(means[..., 1:2], filename + '_dbv')
        save_im_data(means[..., 2:3], filename + '_r2p')
        save_im_data(log_stds, filename + '_logstds')
        return iw_maps
