"""Rate of the fleet deployment loop (sim2sim.FleetInfer) with its flight recorder on, against the loop of the
same job without it -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_record_rate.py [--out profiles/fleet_record_rate.txt] [--parent_root ../parent]

The method is tools/fleet_disturb_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed
graphs of ``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every
measurement from the loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Five graphs per
N, measured by turns within every repeat:

  off              FleetInfer._periods, no recorder, nothing configured: the parent's four launches a period
  on               the same loop with a recorder of depth ``depth``: five launches a period
  disturbed off    a command schedule (a new segment every 10 periods), pushes (a drawn magnitude and direction,
                   first at 20, every 25) and sensor noise at level 1, no recorder: five launches a period
  disturbed on     the same with the recorder: six launches a period
  record alone     duck_fleet_record back to back with itself (a graph of ``chunk`` launches of it)

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the period with the recorder off is checked
against the [min, max] those two runs report, widened by the difference between the two runs' medians.
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
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)


def main() -> int:
    p = parser()
    p.add_argument("--depth", type=int, default=50)
    args = parse("fleet_record_rate.py", p)
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_record_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    say(f"recorder: depth {args.depth}, post 0. disturbed: a command schedule (a segment every 10 periods), pushes "
        "(magnitude in [0.1, 1.0], any direction, first at 20, every 25), noise level 1")
    say()
    say(f"{'robots':>7} {'off us':>22} {'on us':>22} {'added us':>9} {'disturbed off us':>22} {'disturbed on us':>22} "
        f"{'added us':>9} {'record alone us':>16} {'ring MB':>8}")
    cells = command_grid("3x3x3")
    off_period, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        def fleet(disturbed, recording):
            f = FleetInfer("flat_terrain", path, n, device=args.device)
            f.set_commands(cells[np.arange(n) % len(cells)])
            if disturbed:
                f.set_command_schedule(resample_schedule(cells, 600, 10), np.arange(n) % len(cells), 10)
                f.set_pushes(20, 25, (0.1, 1.0), (0.0, 2.0 * np.pi))
                f.set_noise(1.0, seed=1)
            if recording:
                f.set_recorder(args.depth)
            assert f.disturbed() == disturbed and (f.ring is not None) == recording
            return f

        fleets = [fleet(False, False), fleet(False, True), fleet(True, False), fleet(True, True)]
        rec = fleets[1]

        def alone(f=rec):
            for _ in range(chunk):
                f.record()

        graphs = [(f, capture(f, lambda f=f: f._periods(chunk))) for f in fleets] + [(rec, capture(rec, alone))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (f, g) in enumerate(graphs):
                times[k].append(replay_seconds(f, g, reps) / chunk * 1e6)
        off, on, doff, don, alo = (spread(t) for t in times)
        off_period[n] = off
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(off):>22} {fmt(on):>22} {on[0] - off[0]:>+9.1f} {fmt(doff):>22} {fmt(don):>22} "
            f"{don[0] - doff[0]:>+9.1f} {alo[0]:>16.1f} {rec.ring.numel() * 4 / 1e6:>8.1f}")
        del fleets, rec, graphs
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, off_period, "period with the recorder off")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
