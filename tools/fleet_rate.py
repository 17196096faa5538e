"""Rate of the fleet deployment loop (sim2sim.FleetInfer) on the flat scene, against the single-robot
MjInfer of the same job.

    python tools/fleet_rate.py [--out profiles/fleet_rate.txt] [--chunk 50] [--reps 4] [--repeat 3]

For N = 1, 1,024 and 4,096 robots: robot-periods/s of replayed graphs of ``chunk`` control periods, HIP
events around ``reps`` replays after a warm-up replay, every measurement from the loop's start state
(FleetInfer.restart) and repeated ``repeat`` times (median, with the spread). The same way, per period:
duck_physics_step alone (with the aux record) and the other three launches alone (duck_fleet_observe,
duck_policy_act, duck_fleet_actuate); at 4,096 robots duck_physics_step with and without the aux record.
MjInfer.run is timed with the host clock (it synchronises every period). The policy is a seeded,
untrained ActorCritic(101, 212, 14) exported to ONNX: the rates do not depend on its weights, the
trajectories (and so the contact work of the physics) do.
"""

import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, MjInfer  # noqa: E402
from tools.fleet_rate_common import Report, export_policy, parse, parser  # noqa: E402


def graph_seconds(fleet, body, reps: int, repeat: int):
    """Seconds per replay of a graph of ``body()``: [median, min, max] over ``repeat`` measurements."""
    fleet.restart()
    body()                                   # eager once: code objects loaded before the capture
    torch.cuda.synchronize(fleet.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    out = []
    for _ in range(repeat):
        fleet.restart()
        g.replay()                           # the warm-up chunk
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize(fleet.device)
        out.append(e0.elapsed_time(e1) * 1e-3 / reps)
    return statistics.median(out), min(out), max(out)


def main() -> int:
    args = parse("fleet_rate.py", parser(parent_root=False))
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}")

    mj = MjInfer("flat_terrain", onnx_model_path=path, device=args.device)
    mj.run(20)
    t0 = time.perf_counter()
    mj.run(200)
    mj_rate = 200 / (time.perf_counter() - t0)
    say(f"MjInfer.run (1 robot, host loop, 200 periods): {mj_rate:,.0f} periods/s")
    say()
    say(f"{'robots':>7} {'robot-periods/s':>16} {'x MjInfer':>10} {'period us':>22} {'physics us':>11} {'other 3 us':>11}")
    for n in [int(v) for v in args.sizes.split(",")]:
        fleet = FleetInfer("flat_terrain", path, n, device=args.device)

        def physics(fleet=fleet):
            for _ in range(chunk):
                fleet._physics(fleet.decimation)

        def others(fleet=fleet):
            for _ in range(chunk):
                fleet.observe()
                fleet.act()

        full = graph_seconds(fleet, lambda: fleet._periods(chunk), reps, rep)
        phys = graph_seconds(fleet, physics, reps, rep)
        oth = graph_seconds(fleet, others, reps, rep)
        us = [v / chunk * 1e6 for v in full]
        rate = n * chunk / full[0]
        say(f"{n:>7} {rate:>16,.0f} {rate / mj_rate:>10,.1f} {us[0]:>8.1f} [{us[1]:.1f}, {us[2]:.1f}]"
            f" {phys[0] / chunk * 1e6:>11.1f} {oth[0] / chunk * 1e6:>11.1f}")
        if n == max(int(v) for v in args.sizes.split(",")):
            aux = fleet.aux

            class NoAux:   # duck_physics_step(aux = NULL): the same launch without the debug record
                @staticmethod
                def data_ptr():
                    return None
            fleet.aux = NoAux
            lean = graph_seconds(fleet, physics, reps, rep)
            fleet.aux = aux
            again = graph_seconds(fleet, physics, reps, rep)
            a, b = again[0] / chunk * 1e6, lean[0] / chunk * 1e6
            say()
            say(f"duck_physics_step at {n} robots, 10 substeps: with aux {a:.1f} us [{again[1] / chunk * 1e6:.1f}, "
                f"{again[2] / chunk * 1e6:.1f}], without {b:.1f} us [{lean[1] / chunk * 1e6:.1f}, {lean[2] / chunk * 1e6:.1f}]: "
                f"the record costs {100 * (a - b) / b:+.1f} % of the launch, {100 * (a - b) / us[0]:+.1f} % of the period")
        del fleet
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
