"""Builds pcc-rl_amd/lib/libpcc_sim.so from csrc/*.hip with hipcc for gfx950.
hipcc cross-compiles without a GPU, so this also runs in the GPU-less build container."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# one translation unit per kernel family (each kernel is register-allocated on its own) + the C ABI + the PPO caller's kernels
UNITS = ["pcc_sim.hip", "pcc_send.hip", "pcc_send_restart.hip", "pcc_retire.hip", "pcc_small.hip", "pcc_fused.hip", "pcc_noise_sorted.hip", "pcc_snapshot.hip",
         "pcc_policy.hip", "pcc_ppo.hip", "pcc_mlp_tiles_d32.hip", "pcc_mlp_tiles_d64.hip", "pcc_mlp_tiles_d128.hip", "pcc_pbt.hip", "pcc_obsnorm.hip", "pcc_episodes.hip",
         "pcc_rewnorm.hip", "pcc_updiag.hip", "pcc_gradclip.hip", "pcc_streams.hip", "pcc_timelimit.hip", "pcc_objective.hip"]
SRCS = [os.path.join(CSRC, u) for u in UNITS]
HEADERS = [os.path.join(CSRC, h) for h in ("pcc_dev.h", "pcc_kernels.h", "pcc_wave_pass.h", "pcc_send_item.h", "pcc_send_bodies.h", "pcc_retire_env.h", "pcc_policy_dev.h", "pcc_mlp_tiles.h", "pcc_snapshot.h")]
INCLUDE = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIB_DIR, "libpcc_sim.so")
# the same sources with -DPCC_PROFILE=1: per-item timelines, pass counters and the "skip" switches of tools/ -- never the
# product (those switches drop work: wrong results, timing only)
PROFILE_LIB = os.path.join(LIB_DIR, "libpcc_sim_prof.so")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def library_path(profile=False):
    return PROFILE_LIB if profile else LIB


def _stale(lib):
    if not os.path.exists(lib):
        return True
    newest = max(os.path.getmtime(p) for p in SRCS + HEADERS + [os.path.join(INCLUDE, "pcc_sim.h"), os.path.join(INCLUDE, "pcc_policy.h")])
    return os.path.getmtime(lib) < newest


# variant builds the GPU tests run the parity suite through (tests/test_variants.py): code paths that are exact by
# construction but once broke in code generation: the adaptive trigger of regime C; the restart kernel and the
# small-batch kernel cut for 4 wavefronts per SIMD (128 registers: they spill)
VARIANTS = {
    "adaptc": ["-DPCC_ADAPTIVE_C=1"],
    "tight": ["-DPCC_RESTART_OCC=4", "-DPCC_SMALL_OCC=4"],
}


def variant_path(name):
    return os.path.join(LIB_DIR, "libpcc_sim_var_%s.so" % name)


def _parse_resources(text):
    """kernel -> {vgprs, sgprs, scratch, occupancy, vgpr_spills, sgpr_spills} from -Rpass-analysis=kernel-resource-usage."""
    import re
    out, cur = {}, None
    keys = {"VGPRs:": "vgprs", "TotalSGPRs:": "sgprs", "ScratchSize [bytes/lane]:": "scratch", "Occupancy [waves/SIMD]:": "occupancy",
            "VGPRs Spill:": "vgpr_spills", "SGPRs Spill:": "sgpr_spills", "LDS Size [bytes/block]:": "lds"}
    for line in text.splitlines():
        m = re.search(r"remark: [^:]*:\d+:\d+:\s+(.*?)\s+\[-Rpass-analysis", line) or re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur is not None:
            for k, name in keys.items():
                if t.startswith(k):
                    try:
                        out[cur][name] = int(t[len(k):].strip())
                    except ValueError:
                        pass
    return out


def build_library(force=False, verbose=False, profile=False, extra_flags=(), out=None):
    """Compile the HIP library if it is missing or older than its sources; returns its path.
    profile=True builds the tools' variant (libpcc_sim_prof.so, -DPCC_PROFILE=1) instead.  The translation units are
    compiled side by side (one hipcc process each) and linked into one shared object; extra_flags / out are for variant
    builds (e.g. -DPCC_ADAPTIVE_C=1 into another file).  The compiler's per-kernel resource report (registers, scratch,
    spills) is kept next to the library as <lib>.resources.json: tests/test_abi_cpu.py reads it."""
    import json
    lib = out or library_path(profile)
    if not force and not _stale(lib):
        return lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found; cannot build %s" % lib)
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, "obj_" + os.path.splitext(os.path.basename(lib))[0])
    os.makedirs(obj_dir, exist_ok=True)
    flags = (HIPCC_FLAGS + (["-DPCC_PROFILE=1"] if profile else []) + list(extra_flags) +
             ["-I", INCLUDE, "-I", CSRC, "-Rpass-analysis=kernel-resource-usage"])
    procs, objs = [], []
    for src in SRCS:
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        objs.append(obj)
        cmd = [hipcc] + flags + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.PIPE, universal_newlines=True)))
    resources = {}
    for cmd, p in procs:
        _, err = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), err[-4000:]))
        resources.update(_parse_resources(err))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    try:
        names = subprocess.run(["c++filt"], input="\n".join(resources), stdout=subprocess.PIPE, universal_newlines=True).stdout.split("\n")
        resources = {n.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", ""): v for n, v in zip(names, resources.values())}
    except OSError:
        pass
    with open(lib + ".resources.json", "w") as f:
        json.dump(resources, f, indent=1, sort_keys=True)
    with open(lib + ".build_info.json", "w") as f:
        json.dump(_source_stamp(extra_flags, profile), f, indent=1, sort_keys=True)
    return lib


def _source_stamp(extra_flags=(), profile=False):
    """What a built library was compiled from: the commit of the tree (and whether csrc/ or include/ differed from it) -- the GPU
    box gets the built .so but no .git, and every measurement file names the code it measured -- plus a hash of the sources."""
    import hashlib
    import time
    h = hashlib.sha256()
    for p in sorted(SRCS + HEADERS + [os.path.join(INCLUDE, "pcc_sim.h"), os.path.join(INCLUDE, "pcc_policy.h")]):
        with open(p, "rb") as f:
            h.update(f.read())
    stamp = {"sources_sha16": h.hexdigest()[:16], "flags": HIPCC_FLAGS + (["-DPCC_PROFILE=1"] if profile else []) + list(extra_flags),
             "built_at": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "commit": None, "dirty": None}
    try:
        stamp["commit"] = subprocess.run(["git", "rev-parse", "--short=12", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                         universal_newlines=True, timeout=10).stdout.strip() or None
        if stamp["commit"]:
            stamp["dirty"] = bool(subprocess.run(["git", "status", "--porcelain", "--", "pcc-rl_amd/csrc", "include"], cwd=ROOT,
                                                 stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True, timeout=10).stdout.strip())
    except (OSError, subprocess.SubprocessError):
        pass
    return stamp


def build_info(lib=None):
    """The stamp build_library() left next to `lib` (default: the product library); {} if there is none."""
    import json
    try:
        with open((lib or LIB) + ".build_info.json") as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def build_variants(force=False, verbose=False):
    """The variant libraries of VARIANTS (see there) and the test harnesses of rtt_means, of the boundary searches and of the send half's wave passes; returns
    {name: path} of the variants."""
    out = {name: build_library(force=force, verbose=verbose, extra_flags=flags, out=variant_path(name)) for name, flags in VARIANTS.items()}
    build_rtt_harness(force=force, verbose=verbose)
    build_search_harness(force=force, verbose=verbose)
    build_send_harness(force=force, verbose=verbose)
    return out


# tests/kernels/rtt_means_harness.hip: rtt_means<8> and <16> of csrc/pcc_retire_env.h behind one C entry, for tests/test_rtt_means.py.
# A library of its own next to the variants -- never a unit of libpcc_sim.so -- compiled with the product's flags as they are
# (-ffp-contract=off is part of what the routine promises).
RTT_HARNESS_SRC = os.path.join(ROOT, "tests", "kernels", "rtt_means_harness.hip")
RTT_HARNESS_LIB = os.path.join(LIB_DIR, "libpcc_rtt_harness.so")


# tests/kernels/retire_search_harness.hip: search_many, search_boundary, fix_drop_boundary_g and drop_hop1_candidate_g of
# csrc/pcc_retire_env.h, 8 and 16 lanes, behind four C entries, for tests/test_retire_search.py.  Built as the rtt harness is.
SEARCH_HARNESS_SRC = os.path.join(ROOT, "tests", "kernels", "retire_search_harness.hip")
SEARCH_HARNESS_LIB = os.path.join(LIB_DIR, "libpcc_search_harness.so")


def build_rtt_harness(force=False, verbose=False):
    """Compile the harness if it is missing or older than its source or the headers; returns its path -- None, and nothing is
    built, in a tree that has no tests/ (the harness is test infrastructure: the product builds without it)."""
    return _build_harness(RTT_HARNESS_SRC, RTT_HARNESS_LIB, force, verbose)


def build_search_harness(force=False, verbose=False):
    """The same for the harness of the boundary searches and the near-group repairs."""
    return _build_harness(SEARCH_HARNESS_SRC, SEARCH_HARNESS_LIB, force, verbose)


# tests/kernels/send_pass_harness.hip: heavy_mi (a wavefront, staged or not, and a team) and heavy_mi2 (staged or not) of
# csrc/pcc_wave_pass.h, TRACE and Philox, behind two C entries, for tests/test_send_pass_device.py.  Built twice with the
# product's flags: plainly, and with -DPCC_PROFILE=1 (the passes count themselves by regime: what the test's reach check reads).
SEND_HARNESS_SRC = os.path.join(ROOT, "tests", "kernels", "send_pass_harness.hip")
SEND_HARNESS_LIB = os.path.join(LIB_DIR, "libpcc_send_harness.so")
SEND_HARNESS_PROF_LIB = os.path.join(LIB_DIR, "libpcc_send_harness_prof.so")


def build_send_harness(force=False, verbose=False):
    """The same for the harness of the send half's wave passes; returns (plain, profile) paths, or None without tests/."""
    plain = _build_harness(SEND_HARNESS_SRC, SEND_HARNESS_LIB, force, verbose)
    if plain is None:
        return None
    return plain, _build_harness(SEND_HARNESS_SRC, SEND_HARNESS_PROF_LIB, force, verbose, extra_flags=("-DPCC_PROFILE=1",))


def _build_harness(src, lib, force, verbose, extra_flags=()):
    if not os.path.exists(src):
        return None
    if not force and os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(p) for p in [src] + HEADERS):
        return lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found; cannot build %s" % lib)
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [hipcc] + HIPCC_FLAGS + list(extra_flags) + ["-I", INCLUDE, "-I", CSRC, "-shared", src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    p = subprocess.run(cmd, stderr=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    return lib
