"""Dev timing of qbold_elbo_bwd (1 M voxels, S = 1, K = 70 by default): the specialised T = 11 / 24 kernels against
elbo_bwd_generic_kernel under QBOLD_KSEL_ELBO_BWD_GENERIC, interleaved in one process, and the generic kernel on
BASELINE config 3's 64 taus: python scripts/dev/time_elbo_bwd.py [S K] [out.json]"""
import configparser, json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench
GENERIC = 8388608   # QBOLD_KSEL_ELBO_BWD_GENERIC
cfg = configparser.ConfigParser(); cfg.read(os.path.join(ROOT, "config")); base = dict(cfg["DEFAULT"])
nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
S, K = (nums + [1, 70])[:2] if len(nums) >= 2 else (1, 70)
out_json = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
PROTOCOLS = {11: {}, 24: dict(tau_start="-0.028", tau_end="0.065", tau_step="0.004"),
             64: dict(tau_start="-0.015", tau_end="0.065", tau_step="0.00125")}
n = 1 << 20
rows = []
for T, over in PROTOCOLS.items():
    ctx, x = bench.make_inputs(n, dict(base, **over), seed=1, device=torch.device("cuda:0"))
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    prior = torch.tensor([-0.4, -0.3, -2.0, 0.1, 0.0], device="cuda").repeat(n, 1)
    q = prior + 0.3 * torch.randn(n, 5, generator=g, device="cuda")
    ls = torch.full((n, T), -3.5, device="cuda") + 0.2 * torch.randn(n, T, generator=g, device="cuda")
    mask = torch.ones(n, device="cuda")
    sels = [0, GENERIC] if T in (11, 24) else [0]    # every other T runs the generic kernel whatever the selection
    def run(k):
        for _ in range(k):
            r = ctx.elbo_bwd(x, mask, q, prior, ls, S, K, seed=1)
        return r
    t0 = time.time()
    while time.time() - t0 < 0.3:
        run(5); torch.cuda.synchronize()
    for rep in range(3):
        for sel in sels:
            ctx.set_kernel_selection(sel)
            run(5); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 40
            a.record(); r = run(reps); b.record(); torch.cuda.synchronize()
            s = r[0].cpu()
            ms = a.elapsed_time(b) / reps
            kern = "generic" if (sel or T not in (11, 24)) else "specialised"
            rows.append(dict(T=T, S=S, K=K, kernel=kern, rep=rep, ms=ms, neg_elbo=float((s[0] + s[1]) / s[2])))
            print(f"T={T} S={S} K={K} {kern:11s}: {ms:.4f} ms per call (allocations included)   -ELBO {rows[-1]['neg_elbo']:.6f}", flush=True)
if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
