"""Rate of the fleet deployment loop (sim2sim.FleetInfer) with its disturbances on, against the undisturbed
loop of the same job -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_disturb_rate.py [--out profiles/fleet_disturb_rate.txt] [--parent_root ../parent]

The method is tools/fleet_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed graphs of
``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every measurement from
the loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Three graphs per N, measured by
turns within every repeat:

  undisturbed   FleetInfer._periods with nothing configured: four launches a period
  four launches the parent commit's loop written out here: physics, observe, policy, actuate
  disturbed     a command schedule (a new segment every 10 periods), pushes (a drawn magnitude and direction,
                first at 20, every 25) and sensor noise at level 1: five launches a period

and duck_fleet_disturb alone (a graph of ``chunk`` launches of it). ``--parent_root`` names a built checkout
of the parent commit: its tools/fleet_rate.py is run there as a child process before this commit's graphs and
again after them (another process places its buffers and code elsewhere, and the period moves by some tenths
of a microsecond with it), and the undisturbed period is checked against the [min, max] those runs report.
"""

import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native, onnx_export, ppo  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid, resample_schedule  # noqa: E402


def capture(fleet, body):
    fleet.restart()
    body()                                   # eager once: code objects loaded before the capture
    torch.cuda.synchronize(fleet.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g


def replay_seconds(fleet, g, reps: int) -> float:
    fleet.restart()
    g.replay()                               # the warm-up chunk
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize(fleet.device)
    return e0.elapsed_time(e1) * 1e-3 / reps


def spread(v):
    return statistics.median(v), min(v), max(v)


def parent_periods(root: str, sizes: str, chunk: int, reps: int, repeat: int, device: str):
    """{N: (median, min, max) period us} of the parent checkout's tools/fleet_rate.py, and its output."""
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fleet_rate.py"), "--sizes", sizes, "--chunk",
                        str(chunk), "--reps", str(reps), "--repeat", str(repeat), "--device", device], cwd=root,
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"the parent's fleet_rate.py failed:\n{r.stdout}\n{r.stderr}")
    out = {}
    for m in re.finditer(r"^\s*(\d+)\s+[\d,]+\s+[\d,.]+\s+([\d.]+) \[([\d.]+), ([\d.]+)\]", r.stdout, re.M):
        out[int(m.group(1))] = tuple(float(m.group(k)) for k in (2, 3, 4))
    return out, r.stdout


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--chunk", type=int, default=50)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--sizes", default="1,1024,4096")
    p.add_argument("--parent_root", default=None)
    p.add_argument("--device", default="cuda:0")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fleet_disturb_rate.py measures on the GPU; none is available")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(3)
    net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
    net.obs_norm.update(torch.tensor(np.random.default_rng(0).normal(size=(500, 101)), dtype=torch.float32))
    path = os.path.join(tempfile.mkdtemp(), "policy.onnx")
    onnx_export.export_onnx(net, 14, 101, output_path=path)
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_disturb_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    say("disturbed: a command schedule (a segment every 10 periods), pushes (magnitude in [0.1, 1.0], any direction, "
        "first at 20, every 25), noise level 1")
    say()
    say(f"{'robots':>7} {'undisturbed us':>24} {'four launches us':>24} {'disturbed us':>24} {'disturb alone us':>17} {'added us':>9}")
    cells = command_grid("3x3x3")
    undisturbed, runs = {}, []
    if args.parent_root:
        runs.append(parent_periods(os.path.abspath(args.parent_root), args.sizes, chunk, reps, rep, args.device))
    for n in [int(v) for v in args.sizes.split(",")]:
        plain = FleetInfer("flat_terrain", path, n, device=args.device)
        plain.set_commands(cells[np.arange(n) % len(cells)])
        dist = FleetInfer("flat_terrain", path, n, device=args.device)
        dist.set_commands(cells[np.arange(n) % len(cells)])
        dist.set_command_schedule(resample_schedule(cells, 600, 10), np.arange(n) % len(cells), 10)
        dist.set_pushes(20, 25, (0.1, 1.0), (0.0, 2.0 * np.pi))
        dist.set_noise(1.0, seed=1)
        assert dist.disturbed() and not plain.disturbed()

        def four(fleet=plain):
            for _ in range(chunk):
                fleet._physics(fleet.decimation)
                fleet.observe()
                fleet.act()

        def alone(fleet=dist):
            for _ in range(chunk):
                fleet.disturb()

        graphs = [(plain, capture(plain, lambda: plain._periods(chunk))), (plain, capture(plain, four)),
                  (dist, capture(dist, lambda: dist._periods(chunk))), (dist, capture(dist, alone))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (fleet, g) in enumerate(graphs):
                times[k].append(replay_seconds(fleet, g, reps) / chunk * 1e6)
        und, par, dis, alo = (spread(t) for t in times)
        undisturbed[n] = und
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(und):>24} {fmt(par):>24} {fmt(dis):>24} {alo[0]:>17.1f} {dis[0] - und[0]:>+9.1f}")
        del plain, dist, graphs
    if args.parent_root:
        runs.append(parent_periods(os.path.abspath(args.parent_root), args.sizes, chunk, reps, rep, args.device))
        say()
        say("the parent commit's tools/fleet_rate.py, run in its own checkout as a child process of this job, once "
            "before the graphs above and once after them:")
        for k, (_, text) in enumerate(runs):
            for line in text.rstrip().splitlines():
                say(f"  {('before', 'after')[k]} | " + line)
        say()
        for n in sorted(undisturbed):
            u = undisturbed[n]
            each = ", ".join(f"[{r[n][1]:.1f}, {r[n][2]:.1f}]" for r, _ in runs)
            lo, hi = min(r[n][1] for r, _ in runs), max(r[n][2] for r, _ in runs)
            verdict = "inside" if lo <= u[0] <= hi else ("below (faster than)" if u[0] < lo else "ABOVE (slower than)")
            say(f"undisturbed period at {n} robots: {u[0]:.1f} us [{u[1]:.1f}, {u[2]:.1f}]; the parent's two runs {each}: "
                f"{verdict} the parent's [{lo:.1f}, {hi:.1f}]")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
