"""Loader for the MI355X C-ABI library (``libduck.so``, ``include/duck.h``).

The product path only ever calls into this library; there is no CPU fallback. If the
shared object is missing or fails to load, every entry point raises.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

from .cabi import FLEET_GAIT_HEADERS, HEADERS

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DUCK_LIB") or os.path.join(HERE, "libduck.so")
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)

BUILD = os.path.join(HERE, "build")  # libraries compiled for other models (model_library)

# include/*.h through cabi.HEADERS: the structs, the limits and the declared entry points
DuckLayout = HEADERS.structs["duck_layout"]
DuckMlpProblem = HEADERS.structs["duck_mlp_problem"]
DuckGatherField = HEADERS.structs["duck_gather_field"]
DuckFleetDesc = HEADERS.structs["duck_fleet_desc"]
DuckFleetGaitDesc = FLEET_GAIT_HEADERS.structs["duck_fleet_gait_desc"]   # (include/duck_fleet_gait.h)
DuckFleetDisturbance = HEADERS.structs["duck_fleet_disturbance"]
FLEET_MAX_NU = HEADERS.consts["DUCK_FLEET_MAX_NU"]
FLEET_PUSH_SIZE = HEADERS.consts["DUCK_FLEET_PUSH_SIZE"]
FLEET_MAX_DELAY = HEADERS.consts["DUCK_FLEET_MAX_DELAY"]
FLEET_LAT_SIZE = HEADERS.consts["DUCK_FLEET_LAT_SIZE"]
FLEET_LAT_TAG = HEADERS.consts["DUCK_FLEET_LAT_TAG"]
FLEET_ENC_SIZE = HEADERS.consts["DUCK_FLEET_ENC_SIZE"]
EXPORTS = list(HEADERS.funcs)


class DuckError(RuntimeError):
    pass


# the machine scheduler's max-ILP strategy: the step kernel runs one wave per SIMD, so
# occupancy-driven scheduling buys nothing and latency hiding must come from the wave's own
# instruction stream (same-box A/B: +3 % env-steps/s). Every unit uses it; the build is
# gated by tools/isa_exec_check.py, which rejects the register-allocation fault that once made
# the rough + backlash physics_kernel compute a wrong Newton step.
ILP_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"]

# the scene units (variant_*.hip) only. No vector-combine: the LDL' row updates put two adjacent column
# registers into one packed FMA (duck_team.h fac_upd); that pass turns the two scalar reads into a vector load
# of the columns' stack object before it is promoted to registers, which then stays in scratch (flat step
# kernel: 168 scratch instructions, private segment 288 -> 384 bytes). Without the pass: none and 288 bytes,
# and the pass did nothing else in these units (the parent's rough + backlash unit compiles to the same
# assembly with and without it). The learner's GEMM unit changes with the flag and does not get it.
SCENE_FLAGS = ["-mllvm", "-disable-vector-combine"]


def _base_flags(inc: str) -> list:
    # fp32 division and sqrt as v_rcp/v_sqrt (1-2 ulp) instead of the correctly rounded
    # multi-instruction sequences: the physics tolerances are fp32-vs-fp64 anyway; fp32
    # denormals flushed (no frexp/ldexp range scaling around v_rcp/v_sqrt/sincos); x/y as
    # x*rcp(y) and signed zeros ignored (+0.8 % same-box, parity unchanged) -- NaN/Inf stay
    # honoured: the termination check and the auto-reset NaN guard depend on them
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
            "-fgpu-flush-denormals-to-zero", "-fno-slp-vectorize",
            "-fno-signed-zeros", "-fno-trapping-math", "-fno-math-errno", "-freciprocal-math", "-I" + CSRC,
            "-I" + inc]


def compile_flags() -> list:
    """The hipcc flags of the shipped scene units (tools: occupancy_probe.sh, ISA studies)."""
    return _base_flags(os.path.join(CSRC, "generated")) + ILP_FLAGS + SCENE_FLAGS


def build(verbose: bool = False, defines=(), out: str = None, extra_flags=(), no_ilp=(), isa_check: bool = True,
          gen_dir: str = None) -> str:
    """Compile libduck.so for gfx950 with hipcc (in-tree, so it travels with the repo).

    One translation unit per model variant (variant_*.hip) plus the C ABI (duck_capi.hip),
    compiled in parallel and linked into one shared library. ``gen_dir`` (model_library) holds
    the units, headers and variant registry of other models instead of the four shipped scenes.
    One builder per output at a time (torchrun ranks importing the package together): the others
    wait on a file lock and then find the library fresh, so N ranks run one hipcc build, not N."""
    import fcntl
    out = os.path.abspath(out or LIB_PATH)
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, os.path.basename(out) + ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            # the freshness check runs under the lock: a rank never scans a library another rank
            # is still replacing
            return _build_unlocked(verbose, defines, out, extra_flags, no_ilp, isa_check, gen_dir)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_unlocked(verbose, defines, out, extra_flags, no_ilp, isa_check, gen_dir) -> str:
    if gen_dir is None:
        srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
        inc = os.path.join(CSRC, "generated")
    else:
        srcs = [os.path.join(CSRC, "duck_capi.hip")] + \
            sorted(os.path.join(gen_dir, f) for f in os.listdir(gen_dir) if f.endswith(".hip"))
        inc = gen_dir
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
        [os.path.join(inc, f) for f in os.listdir(inc)] + \
        [os.path.join(ROOT, "include", f) for f in sorted(os.listdir(os.path.join(ROOT, "include"))) if f.endswith(".h")] + \
        [os.path.abspath(__file__)]  # the compile flags live here
    # (a define/flag build into the shared output is never "fresh"; a unit directory's own output is)
    if (gen_dir is not None or not defines and not extra_flags) and os.path.exists(out) and \
            os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    import hashlib
    import tempfile
    flags = _base_flags(inc) + [f"-D{d}" for d in defines] + list(extra_flags)
    ilp = ILP_FLAGS
    # build id: sha1 of every source, header and flag that shapes the code (duck_build_id()); the
    # .so itself is not byte-reproducible (object paths), so profiles are keyed by this instead
    h = hashlib.sha1(" ".join(flags + ilp + SCENE_FLAGS + sorted(no_ilp)).encode())
    for d in sorted(set(deps) - {os.path.abspath(__file__)}):
        h.update(os.path.relpath(d, ROOT).encode())
        h.update(open(d, "rb").read())
    flags = flags + [f'-DDUCK_BUILD_ID="{h.hexdigest()}"']
    with tempfile.TemporaryDirectory() as tmp:
        objs, procs = [], []
        for src in srcs:
            obj = os.path.join(tmp, os.path.basename(src) + ".o")
            cmd = ["hipcc"] + flags + ([] if os.path.basename(src) in no_ilp else ilp) + \
                (SCENE_FLAGS if os.path.basename(src).startswith("variant_") else []) + ["-c", "-o", obj, src]
            if verbose:
                print(" ".join(cmd))
            procs.append((src, subprocess.Popen(cmd, cwd=CSRC)))
            objs.append(obj)
        bad = [src for src, p in procs if p.wait() != 0]
        if bad:
            raise DuckError(f"hipcc failed on {bad}")
        # a per-process temporary: concurrent builders (ranks, model_library callers) never link over
        # or scan each other's file; os.replace publishes the checked library atomically
        tmp_out = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-o", tmp_out] + objs, cwd=CSRC)
    try:
        if isa_check:
            nvar = sum(os.path.basename(f).startswith("variant_") for f in srcs)
            bad = isa_exec_faults(tmp_out, min_step_kernels=nvar)
            if bad:
                raise DuckError("register-allocation fault in the compiled kernels (split copies ahead of an exec "
                                "restore, tools/isa_exec_check.py):\n" + "\n".join(bad))
        os.replace(tmp_out, out)
    finally:
        if os.path.exists(tmp_out):
            os.remove(tmp_out)
    return out


def model_library(m, verbose: bool = False) -> str:
    """The library whose kernels are compiled for model ``m``: libduck.so when ``m`` is one of the
    shipped scenes, else ``build/libduck_<fingerprint>.so``, generated and compiled on first use
    (codegen.model_header; the model compiler's structural checks apply). The MI355X analogue of
    MJX re-specialising its program when the MJCF changes: an edited XML needs no hand edits."""
    from . import codegen
    from .cabi import model_fingerprint
    fp = model_fingerprint(m)
    for var, task in codegen.DEFAULT_VARIANTS:
        hdr = os.path.join(CSRC, "generated", f"duck_model_{var}.h")
        if os.path.exists(hdr) and f"FINGERPRINT = 0x{fp:016x}ull" in open(hdr).read():
            return LIB_PATH
    import fcntl
    name = f"m{fp:016x}"
    out = os.path.join(BUILD, f"libduck_{name}.so")
    gen = os.path.join(BUILD, f"gen_{name}")
    os.makedirs(gen, exist_ok=True)
    # one builder per model at a time (torchrun ranks, several envs on the same edited XML): the
    # others wait on the lock and then find the library fresh
    with open(os.path.join(BUILD, f"libduck_{name}.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            # regenerate first: a codegen change that alters the header or unit rewrites it, and
            # build()'s freshness check (sources, headers, include/, native.py) then rebuilds
            files = {f"duck_model_{name}.h": codegen.model_header(m, name),
                     f"variant_{name}.hip": codegen.variant_unit(name, f"duck_model_{name}.h"),
                     "duck_variants.inc": codegen.variant_registry([name])}
            for fn, text in files.items():
                path = os.path.join(gen, fn)
                if not os.path.exists(path) or open(path).read() != text:
                    with open(path, "w") as f:
                        f.write(text)
            return build(verbose=verbose, out=out, gen_dir=gen)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def debug_library(name: str, defines, variants=("flat",), verbose: bool = False) -> str:
    """build/libduck_<name>.so: the shipped scene variants in `variants` compiled with extra `defines`
    (test builds, e.g. DUCK_LAT_FORCE_TIMEOUT for test_gpu_env.py::test_latency_timeout_surfaces).
    One scene instead of four keeps the build short; built by __graft_entry__.build(), never on a GPU box."""
    from . import codegen
    gen = os.path.join(BUILD, f"gen_{name}")
    os.makedirs(gen, exist_ok=True)
    # (the defines are a file of the unit directory: a change of them makes build() recompile)
    files = {"duck_variants.inc": codegen.variant_registry(variants), "defines.txt": "\n".join(defines) + "\n"}
    for v in variants:
        files[f"duck_model_{v}.h"] = open(os.path.join(CSRC, "generated", f"duck_model_{v}.h")).read()
        files[f"variant_{v}.hip"] = codegen.variant_unit(v, f"duck_model_{v}.h")
    for fn, text in files.items():
        path = os.path.join(gen, fn)
        if not os.path.exists(path) or open(path).read() != text:
            with open(path, "w") as f:
                f.write(text)
    return build(verbose=verbose, defines=tuple(defines), out=os.path.join(BUILD, f"libduck_{name}.so"), gen_dir=gen)


def isa_kernels(texts) -> list:
    """The kernel symbols (amdgpu_kernel entry labels) in disassembled code objects."""
    import re
    out = []
    for t in texts:
        out += re.findall(r"^[0-9a-f]+ <(_Z\d+(?:step|physics|reset|randomize)_kernel\w*)>:$", t, re.M)
    return out


def isa_exec_faults(so_path: str, min_step_kernels: int = 1):
    """Blocks of the gfx950 code in so_path whose exec-restoring join starts with AGPR/scratch moves
    (tools/isa_exec_check.py): each is a lane-masked live-range split, i.e. a wrong-result kernel.
    Fails closed: raises DuckError when no code object could be disassembled or fewer than
    min_step_kernels step_kernel / physics_kernel symbols were scanned (a missing fat binary, an
    unbundling failure or a compressed bundle must not pass as "no faults")."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_exec_check", os.path.join(ROOT, "tools", "isa_exec_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    texts = mod.code_objects(so_path)
    kern = isa_kernels(texts)
    nstep = sum("step_kernel" in k for k in kern)
    nphys = sum("physics_kernel" in k for k in kern)
    if not texts or nstep < min_step_kernels or nphys < min_step_kernels:
        raise DuckError(f"ISA gate scanned nothing usable in {so_path}: {len(texts)} code object(s), "
                        f"{nstep} step_kernel / {nphys} physics_kernel symbol(s), {min_step_kernels} expected")
    found = []
    for text in texts:
        found += mod.scan(text, os.path.basename(so_path))
    return [f"{func[:80]}: {len(pre)} move(s) before '{ins}'" for _, func, _, pre, ins in found]


_libs = {}


def lib(path: str = None):
    """Load libduck.so, or the library at ``path`` (raises if it is missing: no fallback path exists)."""
    path = os.path.abspath(path or LIB_PATH)
    if path not in _libs:
        if not os.path.exists(path):
            raise DuckError(f"{path} not built; run __graft_entry__.build() or native.build()")
        L = C.CDLL(path)
        # argtypes and restype of every function the headers declare and this library exports. A declared
        # function may be absent: a model's own library (model_library, debug_library) links duck_capi.hip
        # and its variants only; the learner and policy entry points ship with libduck.so.
        HEADERS.bind(L)
        _libs[path] = L
    return _libs[path]


def check(rc: int, L=None):
    if rc != 0:
        raise DuckError(f"libduck error {rc}: {(L or lib()).duck_last_error().decode()}")
    return rc
