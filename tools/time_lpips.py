"""GPU time of the fit stage's patch terms as HIP kernels (lpips_hip.FusedLPIPS, depth_reg) next to the torch module with autograd, and the
fit stage's iterations per second with the reference's loss weights on both paths.

    python tools/time_lpips.py --out profiles/lpips_timing.txt [--repeat 60] [--steps 120] [--parts a b c]

Weights are seeded stand-ins (He-normal trunk, `lin` uniform in [0, 1)): the pretrained ones cannot be fetched; times do not depend on them.
  a  value and gradient of the LPIPS term for 4 patches of 32 x 32: device events around `FusedLPIPS.value_and_grad` and around the torch
     module's forward + autograd backward, alternating in this one process, `--repeat` (>= 50) times after 10 warm-up rounds: median and
     spread; the launch counts of both (the torch path's from torch.profiler)
  b  one `value_and_grad` and one `depth_reg_value_and_grads` split by C-ABI entry: events around every `_lib.call`, summed per entry
     within a step, median over `--repeat` steps (each figure includes the gap to the next launch)
  c  fit-stage iterations per second (4 frames of 256^2, 4 patches of 32^2, w_lpips = 0.01, w_depth_reg = 0.01) for patch terms "torch"
     and "hip", each eager and replayed from a graph: wall time over `--steps` steps after 20, synchronised at both ends, three trips"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(xs):
    return "%9.1f (%8.1f .. %8.1f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=60)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import copy
    import torch
    import lpips_refs as lr
    from instantavatar_amd import _lib, lpips_hip
    from instantavatar_amd.drivers import fit as fit_driver
    from instantavatar_amd.training import GraphedTrainStep, NGPLoss, configure_optimizer
    if not torch.cuda.is_available():
        sys.exit("time_lpips.py needs the GPU")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    module = lr.seeded_lpips(0).to(dev)
    fused = lpips_hip.FusedLPIPS(module)
    pred, target = (t.to(dev) for t in lr.whole_term_inputs(4, 32, 32, 21))
    say("LPIPS(VGG-16) and depth terms of the patch loss (%s): 4 patches of 32 x 32, fp32" % torch.cuda.get_device_name(0))
    say("floors from the shapes: 7.5 GFLOP at the 157 TFLOP/s fp32 matrix peak = 48 us; 118 MB of weights at 8 TB/s = 15 us")

    def torch_term():
        p = pred.clone().requires_grad_(True)
        pr = p[..., [2, 1, 0]].permute(0, 3, 1, 2).clip(max=1)
        v = module(pr, target[..., [2, 1, 0]].permute(0, 3, 1, 2)).reshape(-1)
        v.sum().backward()
        return v, p.grad

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3
    if "a" in args.parts:
        for _ in range(10):
            fused.value_and_grad(pred, target)
            torch_term()
        torch.cuda.synchronize()
        t_hip, t_torch = [], []
        for _ in range(max(args.repeat, 50)):
            t_hip.append(timed(lambda: fused.value_and_grad(pred, target)))
            t_torch.append(timed(torch_term))
        n_torch = "not counted"
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                torch_term()
                torch.cuda.synchronize()
            n_torch = "%d" % sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0 or getattr(e, "cuda_time_total", 0) > 0)
        except Exception as e:     # (a build without the tracing library)
            n_torch = "not counted (%s)" % type(e).__name__
        say("(a) value and gradient of the term, us between events, median (min .. max) of %d alternating rounds after 10 warm-up rounds" % len(t_hip))
        say("    FusedLPIPS.value_and_grad          %s   %d kernel launches" % (spread(t_hip), fused.launches))
        say("    torch module, forward + autograd   %s   %s kernel launches" % (spread(t_torch), n_torch))
        m_h, m_t = statistics.median(t_hip), statistics.median(t_torch)
        say("    HIP path / torch path by the medians: %.2f (%s)" % (m_h / m_t, "the HIP path is faster" if m_h < m_t else "the HIP path is not faster"))
    if "b" in args.parts:
        alpha, depth = torch.rand(4, 32, 32, device=dev), 2 + torch.rand(4, 32, 32, device=dev)
        per = {}
        real = _lib.call

        def spy(name, *a):
            if name.endswith("_bytes"):
                return real(name, *a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = real(name, *a)
            e1.record()
            cur.append((name, e0, e1))
            return r
        _lib.call = spy
        try:
            for it in range(5 + max(args.repeat, 50)):
                cur = []
                fused.value_and_grad(pred, target)
                lpips_hip.depth_reg_value_and_grads(alpha, depth)
                torch.cuda.synchronize()
                if it >= 5:
                    tot = {}
                    for name, e0, e1 in cur:
                        c, t = tot.get(name, (0, 0.0))
                        tot[name] = (c + 1, t + e0.elapsed_time(e1) * 1e3)
                    for name, (c, t) in tot.items():
                        per.setdefault(name, (c, []))[1].append(t)
        finally:
            _lib.call = real
        say("(b) one step of the HIP path by C-ABI entry: calls per step, us per step summed over the calls, median (min .. max)")
        for name, (c, ts) in sorted(per.items(), key=lambda kv: -statistics.median(kv[1][1])):
            say("    %-22s %3d  %s" % (name, c, spread(ts)))
        say("    sum of the medians: %.1f us" % sum(statistics.median(ts) for _, ts in per.values()))
    if "c" in args.parts:
        opt_w = dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1, w_lpips=0.01, w_depth_reg=0.01)
        rates = {}
        for trip in range(3):
            for terms in ("torch", "hip"):
                for graphed in (False, True):
                    torch.manual_seed(0)
                    frames, body_model, _ = fit_driver.synthetic_frames(dev, res=256, n_frames=4, noise=0.03, patch=32)
                    model = fit_driver.build_fit_model(frames, body_model, dev)
                    opt = configure_optimizer(model, lr=1e-3, smpl_lr=1e-4)
                    loss_fn = NGPLoss(opt_w, lpips=copy.deepcopy(module), patch_terms=terms)
                    model.train()
                    st = GraphedTrainStep(model, opt, loss_fn, enabled=graphed)
                    for it in range(20):
                        st(frames.batch(it % 4, out=st.inputs))
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for it in range(20, 20 + args.steps):
                        out = st(frames.batch(it % 4, out=st.inputs))
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    key = (terms, "graphed" if graphed else "eager")
                    rates.setdefault(key, []).append(args.steps / dt)
                    if graphed and st.capture_error is not None:
                        say("    (%s graphed: capture failed: %s)" % (terms, st.capture_error))
                    assert bool(torch.isfinite(out["loss"])), key
                    del st, model, opt, loss_fn, frames
        say("(c) fit stage, w_lpips = 0.01, w_depth_reg = 0.01, 4 frames of 256^2, 4 patches of 32^2: it/s over %d steps after 20, median (min .. max) of three trips" % args.steps)
        for key, r in rates.items():
            say("    patch terms %-5s %-7s  %s" % (key[0], key[1], spread(r)))
        for mode in ("eager", "graphed"):
            h, t = statistics.median(rates[("hip", mode)]), statistics.median(rates[("torch", mode)])
            say("    %s: hip / torch = %.2f (%s)" % (mode, h / t, "the HIP path is faster" if h > t else "the HIP path is not faster"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
