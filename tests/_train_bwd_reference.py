"""Float64 reference of the encoder training backward (qbold_encoder_train_bwd / qbold_encoder_spatial_bwd): the two-stream
encoder forward of the oracle (qbo_encoder_fwd, qbo_encoder_fwd_spatial) restated in torch, and its vector-Jacobian
product by autograd.  Voxel batches see the 3x3x1 kernels through their centre tap; crop batches [B, X, Y, Z, T] take
'same' 3x3x1 convolutions in x / y with zero padding (no leakage across batch elements or z slices).  Layer norm and
dropout are not restated (their own finite-difference tests cover them).  Test infrastructure (no GPU needed).

vjp() returns d/dw of (sum g_q . q + sum g_ls . log sigma) / sums[2] as a dict in init_weights' names, every relu
pre-activation (to find relu sites near zero, where a float32 forward and this one may take different sides), and
sum_v |delta| of every bias' pre-activation (a bound for bias entries whose terms cancel)."""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("W0", "b0", "Wc", "bc", "Wr1", "br1", "Wr2", "br2", "Wg", "bg", "Wf", "bf", "Ws", "bs")
# the GPU tests' per-tensor tolerance: max |hip - ref| <= EPS max |ref| for every weight tensor
EPS = 1e-5
BLOCK = ("Wc", "bc", "Wr1", "br1", "Wr2", "br2", "Wg", "bg")


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


def forward(w, x, stream=2, geom=False, act="relu", se_idx=2, hi_only_deltas=False, drop_border_tap=False, pre=None):
    """The encoder on torch tensors.  w: name -> tensor (per-block tensors with a leading [L] axis, 'gate_offset' a
    float); x [N, T] (geom False) or [B, X, Y, Z, T] (geom True).  Returns (q, log_sigma or None); pre (a dict) collects
    the relu pre-activations as (tensor, 3x3 convolutions in front of it, tensor whose rms scales it) under 'z0', 'za<l>',
    'zc<l>', 'b<l>', 'zt<l>', and the bias pre-activations ('bias:<name><l>')."""
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


def vjp(w, x, g_q, g_ls=None, sums=None, stream=2, act="relu", se_idx=2, dtype=torch.float64, **planted):
    """d/dw of (sum g_q . q + sum g_ls . log sigma) / sums[2] (sums None: / 1).  w: init_weights' dict (numpy);
    x [N, T] or [B, X, Y, Z, T] (a crop batch); g_q [N, 5], g_ls [N, T] (or None) over the flattened voxels.
    Returns (grads: name -> float64 array, pre: name -> (float64 array of a relu pre-activation, convolutions in front
    of it, its rms scale), bias_abs: bias name ->
    float64 array of sum_v |d/d pre-activation|).  planted: hi_only_deltas / drop_border_tap (defects for the host
    test of the comparison's teeth)."""
    wt = _tensors(w, dtype, True)
    xt = torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    geom = xt.dim() == 5
    pre = {}
    q, ls = forward(wt, xt, stream=stream, geom=geom, act=act, se_idx=se_idx, pre=pre, **planted)
    for k, v in pre.items():
        if k.startswith("bias:"):
            v.retain_grad()
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
    pre_np = {k: (v[0].detach().double().numpy(), v[1], float(v[2].detach().double().pow(2).mean().sqrt()))
              for k, v in pre.items() if not k.startswith("bias:")}
    return grads, pre_np, bias_abs


def outputs(w, x, stream=2, act="relu", se_idx=2):
    """(q, log_sigma) of the float64 forward, numpy."""
    wt = _tensors(w, torch.float64, False)
    xt = torch.tensor(np.asarray(x, np.float64))
    with torch.no_grad():
        q, ls = forward(wt, xt, stream=stream, geom=xt.dim() == 5, act=act, se_idx=se_idx)
    return q.numpy(), None if ls is None else ls.numpy()


def scaled(grads, f):
    """Every entry times f (exact in float64 for a power of two)."""
    return {k: v * f for k, v in grads.items()}


def per_tensor(grads, L):
    """(name, block or None, array) for every weight tensor of the canonical blob."""
    for k in NAMES:
        if k in BLOCK:
            for l in range(L):
                yield k, l, grads[k][l]
        else:
            yield k, None, grads[k]


def error_ratios(got, ref, bias_abs=None, stream=2):
    """max |got - ref| / max |ref| per weight tensor (bias tensors: over max(max |ref|, max sum_v |delta|) when
    bias_abs is given -- their entries can cancel).  Tensors the stream does not reach (ref identically zero) must come
    out zero.  Returns {(name, block): ratio}."""
    L = ref["Wc"].shape[0]
    out = {}
    for name, l, r in per_tensor(ref, L):
        gt = np.asarray(got[name] if l is None else got[name][l], np.float64).reshape(r.shape)
        den = float(np.abs(r).max())
        if bias_abs is not None and name in bias_abs:
            ba = bias_abs[name] if l is None else bias_abs[name][l]
            den = max(den, float(np.max(ba)))
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
        out[name] = np.stack(arrs) if name in BLOCK else arrs[0]
    return out
