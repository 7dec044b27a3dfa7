"""Times the two launches of the device renderer (csrc/ses_render.hip): python tools/time_render.py [--out FILE]

500 recorded BipedalWalker states (20 envs x 25 steps of seeded random actions) and 500 CartPole states, 600 x 400 each: the
scene launch (ses_render_scene) and the raster launch (ses_render_frames) in microseconds per launch, device events around 20
repetitions after 3 warm-up launches, three such windows each (the spread is printed).  As context, where PIL is present: the
same primitive lists drawn on the host with PIL.ImageDraw (polygons, ellipses, thick lines -- PIL's own coverage rules, not the
contract's; a time, not a comparison of pixels).  The output is the record in profiles/render_timing.txt.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))

from ses import HipES  # noqa: E402

REPS, WARMUP, WINDOWS = 20, 3, 3


def record_states(es, n_env, steps, seed, discrete):
    """n_env * steps state blobs of a seeded random walk through the env"""
    init = es.init_states_uniform(seed, 0, 0, n_env)[:, 0].contiguous()
    state, _ = es.env_reset(init)
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        if discrete:
            act = torch.from_numpy(rng.randint(0, es.A, size=n_env).astype(np.int32)).to(es.device)
        else:
            act = torch.from_numpy(np.tanh(rng.randn(n_env, es.A)).astype(np.float32)).to(es.device)
        es.env_step_generic(state, act)
        out.append(state.clone())
    return torch.cat(out)


def time_launch(es, fn):
    """microseconds per launch of fn(): WINDOWS windows of REPS launches between two device events"""
    for _ in range(WARMUP):
        fn()
    es.sync()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(es.stream)
        for _ in range(REPS):
            fn()
        b.record(es.stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / REPS)
    return out


def pil_draw(prims, counts, W, H):
    """seconds to draw the lists with PIL.ImageDraw, or None without PIL"""
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        return None
    t0 = time.perf_counter()
    for f in range(len(counts)):
        im = Image.new("P", (W, H), 0)
        d = ImageDraw.Draw(im)
        for kind, colour, x0, y0, x1, y1, x2, y2 in prims[f, :counts[f]].tolist():
            c = colour & 15
            if kind == 0:
                d.polygon([(x0 / 16, y0 / 16), (x1 / 16, y1 / 16), (x2 / 16, y2 / 16)], fill=c)
            elif kind == 1 and x1 >= 0:
                d.ellipse([(x0 - x1) / 16, (y0 - x1) / 16, (x0 + x1) / 16, (y0 + x1) / 16], fill=c)
            elif kind == 2 and x2 >= 0:
                d.line([(x0 / 16, y0 / 16), (x1 / 16, y1 / 16)], fill=c, width=max(1, round(2 * x2 / 16)))
            elif kind == 3:
                d.rectangle([0, 0, W, H], fill=c)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    lines = [f"device renderer, {torch.cuda.get_device_name(0)}: microseconds per launch, device events around {REPS} launches "
             f"after {WARMUP} warm-up launches, {WINDOWS} windows (median [min .. max])"]
    for name, S, A, discrete in (("BipedalWalker-v3", 24, 4, False), ("CartPole-v1", 4, 2, True)):
        es = HipES(name, S, A, discrete, False, max_step=500, eval_ep_num=1)
        states = record_states(es, 20, 25, 3, discrete)
        W, H = es.render_size()
        prims, counts = es.render_scene(states)
        frames = es.render_frames(prims, counts, W, H)
        es.sync()
        n, mean_count = states.shape[0], float(counts.float().mean())
        scene = time_launch(es, lambda: es.render_scene(states))
        raster = time_launch(es, lambda: es.render_frames(prims, counts, W, H))
        both = time_launch(es, lambda: es.render(states))
        lines.append(f"{name}: {n} states -> {n} frames of {W} x {H}, {mean_count:.1f} primitives a frame, "
                     f"{int(frames.numel()) / 1e6:.0f} MB of frames")
        for what, t in (("scene launch  (ses_render_scene) ", scene), ("raster launch (ses_render_frames)", raster),
                        ("render()      (both, with the allocations of the front end)", both)):
            lines.append(f"  {what}: {np.median(t):9.1f} us  [{min(t):.1f} .. {max(t):.1f}]")
        med = float(np.median(raster))
        lines.append(f"  raster: {med / n:.2f} us a frame, {frames.numel() / med / 1e3:.1f} GB/s of frame bytes, "
                     f"{frames.numel() * mean_count / med / 1e3:.1f} G pixel-primitive pairs/s before culling")
        host = pil_draw(prims.cpu().numpy(), counts.cpu().numpy(), W, H)
        if host is None:
            lines.append("  PIL.ImageDraw: PIL not present, not measured")
        else:
            lines.append(f"  PIL.ImageDraw on the host, the same lists, one thread: {host * 1e6:.0f} us for the {n} frames "
                         f"({host * 1e6 / n:.0f} us a frame) = {host * 1e6 / (np.median(scene) + med):.0f} x the two device launches")
        es.close()
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
