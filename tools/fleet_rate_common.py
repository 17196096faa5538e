"""What the fleet rate tools share (tools/fleet_rate.py and tools/fleet_*_rate.py): the command line, the exported
test policy, the lines that go to the terminal and to ``--out``, graph capture and timed replay, and the check of
this commit's plain period against the parent commit's tools/fleet_rate.py run in the same job. Each tool keeps
its own graphs and its own table."""

import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

from open_duck_playground_amd import onnx_export, ppo


def parser(parent_root: bool = True) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--chunk", type=int, default=50)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--sizes", default="1,1024,4096")
    if parent_root:
        p.add_argument("--parent_root", default=None)
    p.add_argument("--device", default="cuda:0")
    return p


def parse(tool: str, p: argparse.ArgumentParser):
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} measures on the GPU; none is available")
    return args


def export_policy() -> str:
    """The path of a seeded, untrained ActorCritic(101, 212, 14) exported to ONNX: the rates do not depend on its
    weights, the trajectories (and so the contact work of the physics) do."""
    torch.manual_seed(3)
    net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
    net.obs_norm.update(torch.tensor(np.random.default_rng(0).normal(size=(500, 101)), dtype=torch.float32))
    path = os.path.join(tempfile.mkdtemp(), "policy.onnx")
    onnx_export.export_onnx(net, 14, 101, output_path=path)
    return path


class Report:
    """``say(line)`` prints the line and keeps it; ``say.write(path)`` writes the lines kept (no path: nothing)."""

    def __init__(self):
        self.lines = []

    def __call__(self, s=""):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, out):
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                f.write("\n".join(self.lines) + "\n")


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


def parent_run(args):
    """``parent_periods`` of the checkout and the graph sizes a tool's command line names."""
    return parent_periods(os.path.abspath(args.parent_root), args.sizes, args.chunk, args.reps, args.repeat, args.device)


def parent_verdict(say, runs, periods, what: str, widened: bool = True):
    """The parent's two runs (``parent_run`` before and after this commit's graphs), then per N this commit's
    period ``periods[N]`` = (median, min, max) us -- ``what`` names it -- inside, below or ABOVE the [min, max] the
    two runs report, ``widened`` by the distance between their medians."""
    say()
    say("the parent commit's tools/fleet_rate.py, run in its own checkout as a child process of this job, once "
        "before the graphs above and once after them:")
    for k, (_, text) in enumerate(runs):
        for line in text.rstrip().splitlines():
            say(f"  {('before', 'after')[k]} | " + line)
    say()
    for n in sorted(periods):
        u = periods[n]
        widen = abs(runs[0][0][n][0] - runs[1][0][n][0]) if widened else 0.0
        lo, hi = min(r[n][1] for r, _ in runs) - widen, max(r[n][2] for r, _ in runs) + widen
        verdict = "inside" if lo <= u[0] <= hi else ("below (faster than)" if u[0] < lo else "ABOVE (slower than)")
        mine = f"{what} at {n} robots: {u[0]:.1f} us [{u[1]:.1f}, {u[2]:.1f}]; the parent's two runs "
        if widened:
            each = ", ".join(f"{r[n][0]:.1f} [{r[n][1]:.1f}, {r[n][2]:.1f}]" for r, _ in runs)
            say(mine + f"{each}, their medians {widen:.1f} us apart: {verdict} the parent's widened [{lo:.1f}, {hi:.1f}]")
        else:
            each = ", ".join(f"[{r[n][1]:.1f}, {r[n][2]:.1f}]" for r, _ in runs)
            say(mine + f"{each}: {verdict} the parent's [{lo:.1f}, {hi:.1f}]")
