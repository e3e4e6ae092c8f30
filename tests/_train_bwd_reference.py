"""Float64 reference of the encoder training backward (qbold_encoder_train_bwd / qbold_encoder_spatial_bwd): the two-stream
encoder forward of the oracle (qbo_encoder_fwd, qbo_encoder_fwd_spatial) restated in torch, and its vector-Jacobian
product by autograd.  Voxel batches see the 3x3x1 kernels through their centre tap; crop batches [B, X, Y, Z, T] take
'same' 3x3x1 convolutions in x / y with zero padding (no leakage across batch elements or z slices).  use_layer_norm and
dropout_rate (add_normalizer: Dropout, tfa GroupNormalization(groups = 1), then the activation, in front of the residual
path's two convolutions) are restated too: ln [L, 4, U] holds gamma1, beta1, gamma2, beta2 per block, drop [L, 2, rows, U]
the keep factors of a training step (Oracle.dropout_factors: the library's own stream, never restated here).  Test
infrastructure (no GPU needed).

vjp() returns d/dw of (sum g_q . q + sum g_ls . log sigma) / sums[2] as a dict in init_weights' names (plus 'ln'), every
relu pre-activation (to find relu sites near zero, where a float32 forward and this one may take different sides), and
sum_v |delta| of every bias' pre-activation, sum_rows |term| of every GroupNormalization row (bounds for entries whose
terms cancel)."""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("W0", "b0", "Wc", "bc", "Wr1", "br1", "Wr2", "br2", "Wg", "bg", "Wf", "bf", "Ws", "bs")
# the GPU tests' per-tensor tolerance: max |hip - ref| <= EPS max |ref| for every weight tensor
EPS = 1e-5
BLOCK = ("Wc", "bc", "Wr1", "br1", "Wr2", "br2", "Wg", "bg")
LN_ROWS = ("gamma1", "beta1", "gamma2", "beta2")   # the rows of ln[l]; per_tensor's names are 'ln:<row>'
LN_EPS = 1e-3   # tfa GroupNormalization's default epsilon


class _HiOnly(torch.autograd.Function):
    """Identity forward; backward rounds the incoming delta to an f16 high half (11 significant bits) under a
    power-of-two scale that lands its largest magnitude in [2^11, 2^12): what a split that lost its lo half gives."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        m = float(g.abs().max())
        if not m > 0:
            return g
        s = 2.0 ** (12 - np.frexp(m)[1])
        return (g * s).to(torch.float16).to(g.dtype) / s


class _StaleMask(torch.autograd.Function):
    """x keep in the forward; the backward multiplies the delta by another step's keep factors (a planted defect: a
    backward that regenerates the wrong mask)."""

    @staticmethod
    def forward(ctx, x, keep, stale):
        ctx.save_for_backward(stale)
        return x * keep

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def normalise(x, se_idx):
    """normalise_one: log(clip(x) / clip(x)[se_idx]) (one-image normalisation)."""
    c = x.clamp(1e-2, 1e8)
    return torch.log(c / c[..., se_idx:se_idx + 1])


def _act(z, act):
    return torch.relu(z) if act == "relu" else F.gelu(z)


def _conv(a, K, drop_border_tap=False):
    """3x3x1 'same' convolution of a [B, X, Y, Z, U] tensor with K [3, 3, U, U] (Keras orientation: tap (i, j) reads
    the (x + i - 1, y + j - 1) neighbour).  drop_border_tap: a planted defect -- the (+1, 0) tap is lost on the x = 0
    border."""
    B, X, Y, Z, U = a.shape
    p = F.pad(a, (0, 0, 0, 0, 1, 1, 1, 1))
    out = 0
    for i in range(3):
        for j in range(3):
            term = p[:, i:i + X, j:j + Y] @ K[i, j]
            if drop_border_tap and (i, j) == (2, 1):
                keep = torch.ones(X, dtype=a.dtype, device=a.device)
                keep[0] = 0
                term = term * keep[None, :, None, None, None]
            out = out + term
    return out


def forward(w, x, stream=2, geom=False, act="relu", se_idx=2, hi_only_deltas=False, drop_border_tap=False, pre=None,
            ln=None, drop=None, detach_var=False, stale_mask=None):
    """The encoder on torch tensors.  w: name -> tensor (per-block tensors with a leading [L] axis, 'gate_offset' a
    float); x [N, T] (geom False) or [B, X, Y, Z, T] (geom True).  Returns (q, log_sigma or None); pre (a dict) collects
    the relu pre-activations as (tensor, 3x3 convolutions in front of it, tensor whose rms scales it) under 'z0', 'za<l>',
    'zc<l>', 'b<l>', 'zt<l>' ('v1<l>', 'v2<l>': the two normalizers' outputs), the bias pre-activations
    ('bias:<name><l>') and the GroupNormalization rows' terms ('ln:<l>:<which>': (v, xhat)).

    ln [L, 4, U] and / or drop [L, 2, rows, U] (keep factors, rows over the flattened voxels) switch stream 2's residual
    path to train_fwd_impl's normalizer mode: a1 = act(LN1(D1(b))), p = conv1(a1) + br1, a2 = act(LN2(D2(p))),
    r = conv2(a2) + br2 -- no separate act(b); the group of the statistics (biased variance, eps 1e-3) is one voxel for
    [N, T] input and one batch element over X, Y, Z, U for crops.  Planted defects: detach_var (the LN backward
    without its variance term), stale_mask (keep factors [L, 2, rows, U] the backward sees in place of drop's)."""
    pre = {} if pre is None else pre
    L = w["Wc"].shape[0]
    goff = float(w.get("gate_offset", 0.0))
    z0 = normalise(x, se_idx) @ w["W0"] + w["b0"]
    pre["z0"] = (z0, 0, z0)
    pre["bias:b0"] = z0
    h = _act(z0, act)
    a, b = h, h

    def tap(K, l):   # a voxel batch sees the centre tap
        k = K[l]
        return k if k.dim() == 2 else k[1, 1]

    def conv(inp, K, l):
        if not geom:
            return inp @ tap(K, l)
        k = K[l]
        if k.dim() == 2:
            raise ValueError("crops need 9-tap kernels")
        out = _conv(inp, k, drop_border_tap)
        return _HiOnly.apply(out) if hi_only_deltas else out   # the deltas that enter this product

    norm_mode = ln is not None or drop is not None

    def normalizer(xin, l, which, depth):
        u = xin
        if drop is not None:
            keep = drop[l, which].reshape(xin.shape)
            u = xin * keep if stale_mask is None else _StaleMask.apply(xin, keep, stale_mask[l, which].reshape(xin.shape))
        if ln is None:
            # an exact zero (a dropped entry, relu's own zero) is no site: both sides take relu'(0) = 0 there
            pre[f"v{which + 1}{l}"] = (torch.where(u == 0, torch.full_like(u, float("inf")), u), depth, u)
            return _act(u, act)
        dims = tuple(range(1, u.dim())) if geom else (-1,)
        mean = u.mean(dims, keepdim=True)
        var = ((u - mean) ** 2).mean(dims, keepdim=True)
        if detach_var:
            var = var.detach()
        xh = (u - mean) / torch.sqrt(var + LN_EPS)
        v = xh * ln[l, 2 * which] + ln[l, 2 * which + 1]
        pre[f"v{which + 1}{l}"] = (v, depth, v)
        pre[f"ln:{l}:{which}"] = (v, xh.detach())
        return _act(v, act)

    for l in range(L):
        Wc, bc = w["Wc"][l], w["bc"][l]
        if stream == 1:
            za = a @ Wc + bc
            pre[f"za{l}"] = (za, 0, za)
            pre[f"bias:bc{l}"] = za
            a = _act(za, act)
            continue
        zc = b @ Wc + bc
        pre[f"zc{l}"] = (zc, 2 * l, zc)
        pre[f"bias:bc{l}"] = zc
        skip = _act(zc, act)
        if norm_mode:
            zt = conv(normalizer(b, l, 0, 2 * l), w["Wr1"], l) + w["br1"][l]
            pre[f"bias:br1{l}"] = zt
            r = conv(normalizer(zt, l, 1, 2 * l + 1), w["Wr2"], l) + w["br2"][l]
            pre[f"bias:br2{l}"] = r
            gl = r @ w["Wg"][l] + w["bg"][l]
            pre[f"bias:bg{l}"] = gl
            gate = torch.sigmoid(gl + goff)
            b = skip * (1.0 - gate) + r * gate
            continue
        zt = conv(_act(b, act), w["Wr1"], l) + w["br1"][l]
        pre[f"zt{l}"] = (zt, 2 * l + 1, zt)
        pre[f"bias:br1{l}"] = zt
        r = conv(_act(zt, act), w["Wr2"], l) + w["br2"][l]
        pre[f"bias:br2{l}"] = r
        gl = r @ w["Wg"][l] + w["bg"][l]
        pre[f"bias:bg{l}"] = gl
        gate = torch.sigmoid(gl + goff)
        b = skip * (1.0 - gate) + r * gate
        if l + 1 < L:   # the next block's relu(b) (block 0's input is relu(z0) already); b is r gate where skip is 0
            pre[f"b{l + 1}"] = (b, 2 * l + 2, r * gate)
    if stream == 1:
        q = a @ w["Wf"] + w["bf"]
        pre["bias:bf"] = q
        return q, None
    q = b @ w["Wf"] + w["bf"]
    ls = b @ w["Ws"] + w["bs"]
    pre["bias:bf"] = q
    pre["bias:bs"] = ls
    return q, ls


def _tensors(w, dtype, grad):
    out = {}
    for k in NAMES:
        t = torch.tensor(np.asarray(w[k], np.float64), dtype=dtype)
        out[k] = t.requires_grad_(grad)
    out["gate_offset"] = float(w.get("gate_offset", 0.0))
    return out


def _norm_args(ln, drop, stale_mask, dtype, grad):
    lnt = None if ln is None else torch.tensor(np.asarray(ln, np.float64), dtype=dtype).requires_grad_(grad)
    dt = None if drop is None else torch.tensor(np.asarray(drop, np.float64), dtype=dtype)
    st = None if stale_mask is None else torch.tensor(np.asarray(stale_mask, np.float64), dtype=dtype)
    return lnt, dt, st


def vjp(w, x, g_q, g_ls=None, sums=None, stream=2, act="relu", se_idx=2, dtype=torch.float64, ln=None, drop=None,
        stale_mask=None, **planted):
    """d/dw of (sum g_q . q + sum g_ls . log sigma) / sums[2] (sums None: / 1).  w: init_weights' dict (numpy);
    x [N, T] or [B, X, Y, Z, T] (a crop batch); g_q [N, 5], g_ls [N, T] (or None) over the flattened voxels; ln
    [L, 4, U] / drop [L, 2, rows, U]: forward()'s normalizer mode.
    Returns (grads: name -> float64 array ('ln' too when ln is given), pre: name -> (float64 array of a relu
    pre-activation, convolutions in front of it, its rms scale), bias_abs: bias name -> float64 array of
    sum_v |d/d pre-activation|, and 'ln' -> [L, 4, U] of sum_rows |term| (gamma: |d_v xhat|, beta: |d_v|)).  planted:
    hi_only_deltas / drop_border_tap / detach_var / stale_mask (defects for the host test of the comparison's teeth)."""
    wt = _tensors(w, dtype, True)
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    lnt, dt, st = _norm_args(ln, drop, stale_mask, dtype, True)
    geom = xt.dim() == 5
    pre = {}
    q, ls = forward(wt, xt, stream=stream, geom=geom, act=act, se_idx=se_idx, pre=pre, ln=lnt, drop=dt, stale_mask=st,
                    **planted)
    for k, v in pre.items():
        if k.startswith("bias:"):
            v.retain_grad()
        elif k.startswith("ln:"):
            v[0].retain_grad()
    loss = (q.reshape(-1, 5) * torch.tensor(np.asarray(g_q, np.float64), dtype=dtype)).sum()
    if g_ls is not None and ls is not None:
        loss = loss + (ls.reshape(-1, ls.shape[-1]) * torch.tensor(np.asarray(g_ls, np.float64), dtype=dtype)).sum()
    if sums is not None:
        loss = loss / float(sums[2])
    loss.backward()
    grads = {}
    for k in NAMES:
        g = wt[k].grad
        grads[k] = np.zeros(wt[k].shape) if g is None else g.detach().double().numpy()
    if lnt is not None:
        grads["ln"] = np.zeros(lnt.shape) if lnt.grad is None else lnt.grad.detach().double().numpy()
    bias_abs = {}
    for k, v in pre.items():
        if k.startswith("bias:") and v.grad is not None:
            name = k[5:7] if k[5:].startswith(("b0", "bf", "bs")) else k[5:-1]
            a = v.grad.detach().abs().double().reshape(-1, v.shape[-1]).sum(0).numpy()
            if name in BLOCK:
                bias_abs.setdefault(name, []).append(a)
            else:
                bias_abs[name] = a
    bias_abs = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in bias_abs.items()}
    if lnt is not None:
        la = np.zeros(lnt.shape)
        for k, (v, xh) in ((k, v) for k, v in pre.items() if k.startswith("ln:")):
            if v.grad is None:
                continue
            l, which = (int(t) for t in k.split(":")[1:])
            dv = v.grad.detach().double()
            U = dv.shape[-1]
            la[l, 2 * which] = (dv * xh.double()).abs().reshape(-1, U).sum(0).numpy()
            la[l, 2 * which + 1] = dv.abs().reshape(-1, U).sum(0).numpy()
        bias_abs["ln"] = la
    pre_np = {k: (v[0].detach().double().numpy(), v[1], float(v[2].detach().double().pow(2).mean().sqrt()))
              for k, v in pre.items() if not k.startswith(("bias:", "ln:"))}
    return grads, pre_np, bias_abs


def outputs(w, x, stream=2, act="relu", se_idx=2, ln=None, drop=None):
    """(q, log_sigma) of the float64 forward, numpy."""
    wt = _tensors(w, torch.float64, False)
    xt = torch.tensor(np.asarray(x, np.float64))
    lnt, dt, _ = _norm_args(ln, drop, None, torch.float64, False)
    with torch.no_grad():
        q, ls = forward(wt, xt, stream=stream, geom=xt.dim() == 5, act=act, se_idx=se_idx, ln=lnt, drop=dt)
    return q.numpy(), None if ls is None else ls.numpy()


def scaled(grads, f):
    """Every entry times f (exact in float64 for a power of two)."""
    return {k: v * f for k, v in grads.items()}


def per_tensor(grads, L):
    """(name, block or None, array) for every weight tensor of the canonical blob; the GroupNormalization parameters
    (when grads has 'ln') row by row as 'ln:gamma1', 'ln:beta1', 'ln:gamma2', 'ln:beta2'."""
    for k in NAMES:
        if k in BLOCK:
            for l in range(L):
                yield k, l, grads[k][l]
        else:
            yield k, None, grads[k]
    if "ln" in grads:
        for l in range(L):
            for i, row in enumerate(LN_ROWS):
                yield "ln:" + row, l, grads["ln"][l][i]


def _entry(d, name, l):
    if name.startswith("ln:"):
        return d["ln"][l][LN_ROWS.index(name[3:])]
    return d[name] if l is None else d[name][l]


def error_ratios(got, ref, bias_abs=None, stream=2):
    """max |got - ref| / max |ref| per weight tensor (bias tensors and GroupNormalization rows: over
    max(max |ref|, max sum |term|) when bias_abs is given -- their entries can cancel).  Tensors the stream does not
    reach (ref identically zero) must come out zero.  Returns {(name, block): ratio}."""
    L = ref["Wc"].shape[0]
    out = {}
    for name, l, r in per_tensor(ref, L):
        gt = np.asarray(_entry(got, name, l), np.float64).reshape(r.shape)
        den = float(np.abs(r).max())
        if bias_abs is not None and (name in bias_abs or (name.startswith("ln:") and "ln" in bias_abs)):
            den = max(den, float(np.max(_entry(bias_abs, name, l))))
        err = float(np.abs(gt - r).max()) if gt.size else 0.0
        if not np.all(np.isfinite(gt)):
            err = np.inf
        out[(name, l)] = err / den if den > 0 else (0.0 if err == 0 else np.inf)
    return out


def relu_sites_near_zero(pre, rel=1e-5):
    """Int [voxels] (flattened over every leading axis): -1, or the largest reach of a relu site of that voxel whose
    pre-activation lies within rel x its tensor's rms of zero.  A flip there moves the forward through the 3x3
    convolutions after it and the deltas of every voxel within that many convolutions: reach = 2 L - (convolutions in
    front of the site)."""
    L = 1 + max(c for _, c, _ in pre.values()) // 2
    reach = None
    for z, c, rms in pre.values():
        hit = (np.abs(z.reshape(-1, z.shape[-1])) < rel * rms).any(1)
        r = np.where(hit, 2 * L - c, -1)
        reach = r if reach is None else np.maximum(reach, r)
    return reach


def keep_mask(reach, geom=None):
    """Voxels whose head gradients stay: all but the voxels of near-zero relu sites (voxel batches) or, on crops
    geom = (B, X, Y, Z), all but those within Chebyshev distance `reach` in x / y of such a site (same batch element,
    same z)."""
    if geom is None:
        return reach < 0
    B, X, Y, Z = geom
    rr = reach.reshape(B, X, Y, Z)
    hit = np.zeros((B, X, Y, Z), bool)
    for r in range(int(rr.max()) + 1):
        t = torch.tensor((rr == r).astype(np.float32)).permute(0, 3, 1, 2).reshape(B * Z, 1, X, Y)
        d = F.max_pool2d(t, kernel_size=2 * r + 1, stride=1, padding=r)
        hit |= d.reshape(B, Z, X, Y).permute(0, 2, 3, 1).numpy() > 0
    return ~hit.reshape(-1)


def to_arrays(flat, slices):
    """The canonical blob (a float array) as init_weights' dict, per-block tensors stacked, through
    EncoderWeights._slices()."""
    flat = np.asarray(flat, np.float64)
    out = {}
    for name, pieces in slices.items():
        arrs = [flat[off:off + int(np.prod(shape))].reshape(shape) for off, shape in pieces]
        out[name] = np.stack(arrs) if name in BLOCK or name == "ln" else arrs[0]
    return out


# ---- the normalizer cases of tests/test_gpu_train_bwd_normalizer.py (the host test checks their relu bands) ----------
# name: (batch shape, stream, activation, layer norm, dropout rate, U, L, channel-wise gate, weight seed, input seed).
# A relu + layer-norm crop case carries seeds at which the float64 forward has no relu site within 1e-5 rms of zero (the
# group sums carry every voxel's delta to every site of its crop, so no head-gradient screen isolates a flipped site).
NORM_CASES = {
    "v-ln-relu": ((777,), 2, "relu", True, 0.0, 60, 2, True, 5, 4),
    "v-ln-gelu-wide": ((333,), 2, "gelu", True, 0.0, 200, 1, False, 5, 4),
    "v-ln-drop-65": ((501,), 2, "relu", True, 0.25, 65, 2, True, 5, 4),
    "v-drop-128": ((400,), 2, "gelu", False, 0.3, 128, 1, True, 5, 4),
    "v-ln-stride": ((16389,), 2, "gelu", True, 0.0, 20, 2, True, 5, 4),
    "v-gelu": ((1000,), 2, "gelu", False, 0.0, 80, 2, True, 5, 4),
    "v-gelu-s1": ((501,), 1, "gelu", False, 0.0, 128, 1, True, 5, 4),
    "v-ln-s1": ((501,), 1, "relu", True, 0.0, 60, 2, True, 5, 4),
    "c-ln-gelu": ((2, 12, 11, 4), 2, "gelu", True, 0.0, 60, 2, True, 5, 4),
    "c-ln-relu": ((3, 1, 9, 8), 2, "relu", True, 0.0, 64, 1, True, 5, 4),
    "c-ln-drop-relu": ((3, 5, 4, 2), 2, "relu", True, 0.2, 20, 2, True, 5, 4),
    "c-drop-odd": ((4, 9, 1, 4), 2, "gelu", False, 0.5, 33, 1, False, 5, 4),
    "c-gelu": ((3, 12, 11, 4), 2, "gelu", False, 0.0, 60, 2, True, 5, 4),
    "c-rows": ((300, 1, 1, 1), 2, "relu", True, 0.0, 24, 2, True, 5, 4),
}
# TrainState's seed of the first training step (dropout_base + step + 1): the band of c-ln-drop-relu is measured under it
FIRST_STEP_SEED = 0x5eed0001


def norm_weights(U, L, cw, seed, gate_offset=-1.0):
    """(weights, ln [L, 4, U]) as test_gpu_normalizer.make draws them: biases 0.1 N(0, 1), gamma 1 +- 0.3, beta +- 0.2."""
    from oracle.oracle import init_weights
    w = init_weights(T=11, U=U, L=L, channelwise_gating=cw, seed=seed, taps=9, resid_init_std=0.08)
    rng = np.random.default_rng(seed)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = gate_offset
    ln = np.stack([np.stack([1.0 + 0.3 * rng.standard_normal(U), 0.2 * rng.standard_normal(U),
                             1.0 + 0.3 * rng.standard_normal(U), 0.2 * rng.standard_normal(U)]) for _ in range(L)])
    return w, ln.astype(np.float32)


def norm_case(name, oracle32):
    """(weights, ln or None, x) of a NORM_CASES entry; the signals come from the float32 oracle, as the GPU sees them."""
    from oracle.oracle import synth_inputs
    shape, _, _, layer_norm, _, U, L, cw, wseed, xseed = NORM_CASES[name]
    w, ln = norm_weights(U, L, cw, wseed)
    x, _ = synth_inputs(int(np.prod(shape)), seed=xseed, oracle=oracle32)
    return w, (ln if layer_norm else None), x.reshape(*shape, 11)


def drop_factors(oracle, rate, seed, L, rows, U):
    """Keep factors [L, 2, rows, U] of a training step, or None (rate 0): normalizer `which` of block l is the
    stream's layer 2 l + which."""
    if not rate > 0:
        return None
    return np.stack([np.stack([oracle.dropout_factors(rate, seed, 2 * l + which, rows, U) for which in range(2)])
                     for l in range(L)]).astype(np.float64)


def band_is_empty(pre):
    """No relu site of any kind within 1e-5 rms of zero."""
    return bool((relu_sites_near_zero(pre) < 0).all())
