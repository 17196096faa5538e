"""Rate of the fleet deployment loop (sim2sim.FleetInfer) with a joint-encoder delay, against the loop of the same
job with an IMU delay only and with no latency -- and, with ``--parent_root``, against a checkout of the parent
commit in that job.

    python tools/fleet_encoder_rate.py [--out profiles/fleet_encoder_rate.txt] [--parent_root ../parent]

The method is tools/fleet_latency_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed
graphs of ``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every
measurement from the loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Seven graphs per
N, measured by turns within every repeat:

  off              FleetInfer._periods, nothing configured: the parent's four launches a period
  imu, old entry   an IMU delay drawn per robot and period over 0..2, no action delay: five launches a period,
                   duck_fleet_sense_delay after duck_fleet_observe (the loop without an encoder delay)
  imu, new entry   the same table and an all-zero encoder table forced through duck_fleet_sensor_delay in that
                   place: five launches a period, and the policy sees the same bits, so the robots move exactly
                   as in the graph before: the difference is what the new entry costs in the old one's place
  imu + encoder    both delays drawn over 0..2 through duck_fleet_sensor_delay: five launches a period (the robots
                   move otherwise, so this period holds other physics work as well)
  encoder          the encoder delay alone, drawn over 0..2: five launches a period
  sense alone      duck_fleet_sense_delay back to back with itself (a graph of ``chunk`` launches of it)
  sensor alone     duck_fleet_sensor_delay back to back with itself, both delays drawn

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the period with the latency off is checked
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
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)


def main() -> int:
    args = parse("fleet_encoder_rate.py", parser())
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_encoder_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    say("latency: delays drawn per robot and period over 0..2 (every lane evaluates the threefry blocks), seed 1, no action delay")
    say()
    say(f"{'robots':>7} {'off us':>22} {'imu, old entry us':>22} {'added us':>9} {'imu, new entry us':>22} {'new - old us':>13} "
        f"{'imu + encoder us':>22} {'added us':>9} {'encoder us':>22} {'added us':>9} "
        f"{'sense alone us':>15} {'sensor alone us':>16}")
    cells = command_grid("3x3x3")
    off_period, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        def fleet(sense, encoder, forced=False):
            f = FleetInfer("flat_terrain", path, n, device=args.device)
            f.set_commands(cells[np.arange(n) % len(cells)])
            f.set_latency(0, sense, seed=1, encoder=encoder)
            if forced:   # the all-zero encoder table through the new entry
                f.enc = torch.zeros(n, 2, dtype=torch.int32, device=f.device)
                f.eline = torch.zeros(n, 3, 2 * f.num_dofs, dtype=torch.float32, device=f.device)
                f.lat_encoder = True
            assert f.lat_encoder == (forced or encoder != 0) and f.lat_sense == (sense != 0)
            return f

        fleets = [fleet(0, 0), fleet((0, 2), 0), fleet((0, 2), 0, forced=True), fleet((0, 2), (0, 2)), fleet(0, (0, 2))]
        old, both = fleets[1], fleets[3]

        def alone(call):
            def body():
                for _ in range(chunk):
                    call()
            return body

        graphs = [(f, capture(f, lambda f=f: f._periods(chunk))) for f in fleets] + \
            [(old, capture(old, alone(old.sense_delay))), (both, capture(both, alone(both.sensor_delay)))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (f, g) in enumerate(graphs):
                times[k].append(replay_seconds(f, g, reps) / chunk * 1e6)
        off, imu_old, imu_new, two, enc, s_alone, e_alone = (spread(t) for t in times)
        off_period[n] = off
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(off):>22} {fmt(imu_old):>22} {imu_old[0] - off[0]:>+9.1f} {fmt(imu_new):>22} "
            f"{imu_new[0] - imu_old[0]:>+13.1f} {fmt(two):>22} {two[0] - off[0]:>+9.1f} {fmt(enc):>22} {enc[0] - off[0]:>+9.1f} "
            f"{s_alone[0]:>15.1f} {e_alone[0]:>16.1f}")
        del fleets, old, both, graphs
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, off_period, "period with the latency off")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
