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

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid, resample_schedule  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_periods, parent_run,  # noqa: E402, F401
                                     parent_verdict, parse, parser, replay_seconds, spread)


def main() -> int:
    args = parse("fleet_disturb_rate.py", parser())
    say, path = Report(), export_policy()
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
        runs.append(parent_run(args))
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
        runs.append(parent_run(args))
        parent_verdict(say, runs, undisturbed, "undisturbed period", widened=False)
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
