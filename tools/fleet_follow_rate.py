"""Rate of the fleet deployment loop (sim2sim.FleetInfer) following a log, against the loop of the same job with the
policy -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_follow_rate.py [--out profiles/fleet_follow_rate.txt] [--parent_root ../parent]

The method is tools/fleet_latency_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed graphs
of ``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every measurement from the
loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Four graphs per N, measured by turns
within every repeat:

  policy           FleetInfer._periods with no log set: the parent's four launches a period
  following        the same fleet's own closed-loop record followed (a log per command cell, made by a 27-robot
                   closed-loop run of the same policy): four launches a period, duck_fleet_follow in
                   duck_policy_act's place, and the robots move exactly as with the policy (the same physics work)
  policy alone     duck_policy_act back to back with itself (a graph of ``chunk`` launches of it)
  follow alone     duck_fleet_follow back to back with itself, inside the log

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the period with no log set is checked against the
[min, max] those two runs report, widened by the difference between the two runs' medians.
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid, log_from_saved_obs  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)


def main() -> int:
    args = parse("fleet_follow_rate.py", parser())
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    rows = chunk * (reps + 2)          # the eager body before a capture or the warm-up replay, then the timed replays
    say(f"fleet_follow_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    cells = command_grid("3x3x3")
    made = FleetInfer("flat_terrain", path, len(cells), device=args.device)
    made.set_commands(cells)
    log = log_from_saved_obs(np.ascontiguousarray(made.run(rows + 1, record=True).transpose(1, 0, 2)))
    del made
    say(f"following: {len(cells)} logs of {rows} rows, the closed-loop record of the same policy per command cell, robot r "
        f"on log r mod {len(cells)}: the followers move as the policy's robots do")
    say()
    say(f"{'robots':>7} {'policy us':>22} {'following us':>22} {'added us':>9} {'policy alone us':>16} {'follow alone us':>16}")
    no_log, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        plain = FleetInfer("flat_terrain", path, n, device=args.device)
        plain.set_commands(cells[np.arange(n) % len(cells)])
        foll = FleetInfer("flat_terrain", path, n, device=args.device, follow=(log, None))
        assert foll.following() and not plain.following()

        def alone(call):
            def body():
                for _ in range(chunk):
                    call()
            return body

        graphs = [(plain, capture(plain, lambda: plain._periods(chunk))), (foll, capture(foll, lambda: foll._periods(chunk))),
                  (plain, capture(plain, alone(plain.policy))), (foll, capture(foll, alone(foll.follow)))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (f, g) in enumerate(graphs):
                times[k].append(replay_seconds(f, g, reps) / chunk * 1e6)
                assert f is plain or int(f.log_tick.max()) <= rows        # the followers stayed inside the log
        pol, fol, p_alone, f_alone = (spread(t) for t in times)
        no_log[n] = pol
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(pol):>22} {fmt(fol):>22} {fol[0] - pol[0]:>+9.1f} {p_alone[0]:>16.1f} {f_alone[0]:>16.1f}")
        del plain, foll, graphs
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, no_log, "period with no log set")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
