"""Rate of the fleet deployment loop (sim2sim.FleetInfer) with the gait record kept, against the plain loop of the
same job -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_gait_rate.py [--out profiles/fleet_gait_rate.txt] [--parent_root ../parent]

The method is tools/fleet_encoder_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed
graphs of ``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every
measurement from the loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Three graphs per
N, measured by turns within every repeat:

  off          FleetInfer._periods, nothing configured: the parent's four launches a period
  gait         the same loop with the gait record kept: five launches a period, duck_fleet_gait after
               duck_fleet_actuate (the launch reads the loop and writes its own record only, so the robots move
               exactly as in the graph before: the difference is what the launch costs)
  gait alone   duck_fleet_gait back to back with itself (a graph of ``chunk`` launches of it)

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the period with the gait record off is checked
against the [min, max] those two runs report, widened by the difference between the two runs' medians. What the
record costs when kept is reported, not barred.
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)


def main() -> int:
    args = parse("fleet_gait_rate.py", parser())
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_gait_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    say("gait: thresholds at 0.9 of the force limits and at 5.24 rad/s")
    say()
    say(f"{'robots':>7} {'off us':>22} {'gait us':>22} {'added us':>9} {'gait alone us':>22}")
    cells = command_grid("3x3x3")
    off_period, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        def fleet(gait):
            f = FleetInfer("flat_terrain", path, n, device=args.device, gait=(True,) if gait else None)
            f.set_commands(cells[np.arange(n) % len(cells)])
            assert f.gaited() == gait
            return f

        plain, gaited = fleet(False), fleet(True)

        def alone():
            for _ in range(chunk):
                gaited.gait()

        graphs = [(plain, capture(plain, lambda: plain._periods(chunk))), (gaited, capture(gaited, lambda: gaited._periods(chunk))),
                  (gaited, capture(gaited, alone))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (f, g) in enumerate(graphs):
                times[k].append(replay_seconds(f, g, reps) / chunk * 1e6)
        off, on, back = (spread(t) for t in times)
        off_period[n] = off
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(off):>22} {fmt(on):>22} {on[0] - off[0]:>+9.1f} {fmt(back):>22}")
        del plain, gaited, graphs
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, off_period, "period with the gait record off")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
