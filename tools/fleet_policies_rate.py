"""Rate of the fleet deployment loop (sim2sim.FleetInfer) holding several policies, against the plain loop of the
same job -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_policies_rate.py [--out profiles/fleet_policies_rate.txt] [--parent_root ../parent]

The method is tools/fleet_follow_rate.py's: N robots (``--sizes``, default 4,096) on the flat scene, replayed graphs of
``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every measurement from the
loop's start state (FleetInfer.restart), median [min, max] of ``repeat``, all graphs of one N measured by turns
within every repeat. The cases:

  plain            a ``str`` policy path: duck_policy_act, the parent's four launches a period
  K = 1, 8, 64     a list of K distinct policies of the same architecture (K seeds), equal segments:
                   duck_policy_act_multi in duck_policy_act's place, under each block order
                   (duck_policy_multi_order: 0 policy-major, 1 dealt over the XCDs)

and per case two graphs: the whole period, and the policy launch alone, back to back with itself (a graph of
``chunk`` launches of it). A captured launch keeps the order it was enqueued with, so both orders are measured
in the same turns.

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the plain period is checked against the [min, max]
those two runs report, widened by the difference between the two runs' medians. Nothing else has a bar: what
K = 8 and K = 64 cost over K = 1 is reported.
"""

import os
import pathlib
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native, onnx_export, ppo  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)

ORDERS = ((0, "policy-major"), (1, "dealt over XCDs"))


def export_policies(k: int) -> list:
    """K seeded, untrained ActorCritic(101, 212, 14) policies exported to ONNX, distinct weights and normalisers."""
    d = pathlib.Path(tempfile.mkdtemp())
    paths = []
    for seed in range(k):
        torch.manual_seed(100 + seed)
        net = ppo.ActorCritic(101, 212, 14, ppo.PPOConfig())
        net.obs_norm.update(torch.tensor(np.random.default_rng(seed).normal(size=(500, 101)), dtype=torch.float32))
        paths.append(str(d / f"policy_{seed}.onnx"))
        onnx_export.export_onnx(net, 14, 101, output_path=paths[-1])
    return paths


def main() -> int:
    p = parser()
    p.set_defaults(sizes="4096")
    p.add_argument("--policies", default="1,8,64", help="the K to measure")
    args = parse("fleet_policies_rate.py", p)
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    L = native.lib()
    Ks = [int(v) for v in args.policies.split(",")]
    files = export_policies(max(Ks))
    say(f"fleet_policies_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {L.duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    pol = FleetInfer("flat_terrain", path, 1, device=args.device)._policy_args
    sizes = list(pol[1])
    words = sum(a * b + b for a, b in zip(sizes, sizes[1:]))
    say(f"policy layers {sizes}: {4 * words / 1e6:.2f} MB of weights and biases per policy; K distinct policies, equal segments")
    cells = command_grid("3x3x3")
    was = L.duck_policy_multi_order(-1)
    plain_period, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        def fleet(paths):
            f = FleetInfer("flat_terrain", paths, n, device=args.device)
            f.set_commands(cells[np.arange(n) % len(cells)])
            return f

        def alone(f):
            def body():
                for _ in range(chunk):
                    f.policy()
            return body

        plain = fleet(path)
        cases = [("plain (duck_policy_act)", plain, capture(plain, lambda: plain._periods(chunk)), capture(plain, alone(plain)))]
        for K in Ks:
            if n % K:
                say(f"(K = {K} does not divide {n} robots: left out)")
                continue
            f = fleet(files[:K])
            assert f.num_policies == K and f._multi_args is not None
            for o, name in ORDERS:
                L.duck_policy_multi_order(o)
                cases.append((f"K = {K}, {name}", f, capture(f, lambda f=f: f._periods(chunk)), capture(f, alone(f))))
        L.duck_policy_multi_order(was)
        times = [([], []) for _ in cases]
        for _ in range(rep):
            for k, (_, f, g_period, g_alone) in enumerate(cases):
                times[k][0].append(replay_seconds(f, g_period, reps) / chunk * 1e6)
                times[k][1].append(replay_seconds(f, g_alone, reps) / chunk * 1e6)
        say()
        say(f"{n} robots")
        say(f"{'case':>28} {'period us':>24} {'over plain us':>14} {'policy launch alone us':>26} {'over plain us':>14}")
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        base = None
        for (name, *_), (tp, ta) in zip(cases, times):
            sp, sa = spread(tp), spread(ta)
            base = base or (sp, sa)
            say(f"{name:>28} {fmt(sp):>24} {sp[0] - base[0][0]:>+14.1f} {fmt(sa):>26} {sa[0] - base[1][0]:>+14.1f}")
        plain_period[n] = spread(times[0][0])
        del plain, cases
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, plain_period, "plain period (a str policy path)")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
