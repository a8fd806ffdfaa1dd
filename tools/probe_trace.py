#!/usr/bin/env python
"""Per-phase cycle table of the compile-time-geometry half-step kernel (k_half_fused_geo) on a bench workload's batch
(developer tool; the stamps exist only in a -DGNF_TRACE build of the library, which this tool keeps OUTSIDE the package
directory - the shipped libgnf_hip.so has none of it):

    python tools/probe_trace.py --build            # compile build/gnf_trace/libgnf_hip_trace.so (no GPU needed)
    python tools/probe_trace.py [--reps 20]        # run on the GPU box: forward steps of config 2, the table on stdout
    python tools/probe_trace.py --parent           # the same for the one-net-per-wave instance (force_shape = 13)
    python tools/probe_trace.py --build --src-root <another checkout> --out <dir>, then --lib <dir>/libgnf_hip_trace.so
                                                   # the same table for another state of the sources

With GNF_TRACE every wave of the kernel stamps s_memtime (shader cycles) at: kernel entry, behind barrier 1, behind the col
barrier, behind the gather barrier, when the operands of each layer's first MFMA have landed, behind each layer barrier,
behind the coupling store and at the kernel's end; the 8 waves of workgroup 0 and of the mid-grid workgroup copy their stamps
to a buffer of their own.  A phase's figure is the mean over the 8 waves of a workgroup, then the median over launches and
repetitions.  Stamps cost 7 - 11 % of the kernel: compare stamped runs with stamped runs only.

The phased instance (automatic dispatch; phases S0 T0 S1 T1 ..: both nets in every wave) stamps each phase's first MFMA, behind
each phase's barrier, where the last pending tile's store has been issued, and behind the two closing barriers: phases_phased().
"Stage 0 + flush -> behind its barrier" includes the time a wave waits for the wave it shares its SIMD with, which is still
in the previous phase: it is a wave's time, not the matrix pipe's."""
import argparse
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, WAVES, COUPLED, END = 32, 8, 30, 31
PH_FLUSHED = 20        # phased instance (kTracePhFlushed, gnf_fused.hip)
FORCE_GEO_PARENT = 13  # gnf_set_option("force_shape", 13): the one-net-per-wave instance (kForceGeoParent, gnf_options.h)


def build(src_root, out):
    csrc = os.path.join(src_root, "graph-normalizing-flows_amd", "csrc")
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DGNF_TRACE", "-I", os.path.join(src_root, "include"), "-I", csrc]
    os.makedirs(os.path.join(out, "obj"), exist_ok=True)
    from concurrent.futures import ThreadPoolExecutor

    def one(src):
        obj = os.path.join(out, "obj", os.path.basename(src)[:-4] + ".o")
        subprocess.run([hipcc] + flags + ["-c", src, "-o", obj], check=True)
        return obj
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        objs = list(ex.map(one, srcs))
    lib = os.path.join(out, "libgnf_hip_trace.so")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib], check=True)
    print("built", lib)


def phases(k):
    names = [(0, 1, "entry -> barrier 1 (rowptr in LDS)"), (1, 2, "-> col barrier"), (2, 3, "-> gather barrier")]
    prev = 3
    for j in range(k):
        names.append((prev, 4 + 2 * j, f"-> layer {j} operands landed"))
        names.append((4 + 2 * j, 5 + 2 * j, f"layer {j}: first MFMA -> layer barrier"))
        prev = 5 + 2 * j
    names += [(prev, COUPLED, "-> coupling store"), (COUPLED, END, "-> kernel end (reduction)"), (0, END, "entry -> kernel end")]
    return names


def phases_phased(k):
    """The phased instance (automatic dispatch): phase p = 2 j + net of S0 T0 S1 T1 ..; slot 4 + 2 p its first MFMA, 5 + 2 p
    behind its barrier (none in S0), PH_FLUSHED the last pending store issued, then the two closing barriers."""
    names = [(0, 1, "entry -> barrier 1 (rowptr in LDS)"), (1, 2, "-> col barrier"), (2, 3, "-> gather barrier")]
    prev = 3
    for p in range(2 * (k - 1)):
        tag = f"{'ST'[p & 1]}{p >> 1}"
        names.append((prev, 4 + 2 * p, f"-> {tag} first MFMA"))
        prev = 4 + 2 * p
        if p:
            names.append((prev, 5 + 2 * p, f"{tag}: stage 0 + flush -> behind its barrier"))
            prev = 5 + 2 * p
    names += [(prev, PH_FLUSHED, f"-> T{k - 2} done, its flush issued"), (PH_FLUSHED, PH_FLUSHED + 1, "-> behind the flush barrier"),
              (PH_FLUSHED + 1, PH_FLUSHED + 2, "thin chunks -> closing barrier"), (PH_FLUSHED + 2, COUPLED, "-> coupling store"),
              (COUPLED, END, "-> kernel end (reduction)"), (3, PH_FLUSHED + 2, "MLP: gather barrier -> closing barrier"), (0, END, "entry -> kernel end")]
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--src-root", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "gnf_trace"))
    ap.add_argument("--lib", default=None)
    ap.add_argument("--workload", default="config2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent", action="store_true", help="the one-net-per-wave instance (force_shape = 13) and its table")
    args = ap.parse_args()
    if args.build:
        build(os.path.abspath(args.src_root), os.path.abspath(args.out))
        return
    os.environ["GNF_LIB_PATH"] = os.path.abspath(args.lib or os.path.join(args.out, "libgnf_hip_trace.so"))
    sys.path.insert(0, ROOT)
    import torch
    import bench
    bench.WORKLOAD = bench.WORKLOADS[args.workload]
    bench.GRAPHS_PER_GPU = bench.WORKLOAD["graphs"]
    bench.HP.update(bench.WORKLOAD["hp"])
    from gnf_amd import _abi
    from gnf_amd.factories import make_product_grevnet
    from gnf_amd.flow import forward_shard_sums
    from gnf_amd.graphs import build_csr_device, data_dicts_to_graphs_tuple
    lib = _abi.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dicts, n_global, _ = bench.make_batch(1, 0)
    graph = data_dicts_to_graphs_tuple(dicts, dev)
    net = make_product_grevnet(bench.HP, bench.make_params(bench.WEIGHT_SEED, bench.HP, bench.FINAL_SCALE))
    net.fused = True
    build_csr_device(graph)
    launches = 2 * bench.HP["T"]
    k = bench.HP["K"]
    buf = torch.zeros(launches, 2, WAVES, SLOTS, dtype=torch.int64, device=dev)
    lib.gnf_trace_set_buffer.argtypes = [C.c_void_p, C.c_int]
    lib.gnf_trace_set_buffer.restype = None
    for _ in range(5):   # warm-up, not recorded
        forward_shard_sums(net, graph)
    torch.cuda.synchronize()
    _abi.set_option("force_shape", FORCE_GEO_PARENT if args.parent else 0)
    table = phases(k) if args.parent else phases_phased(k)
    if args.parent:
        table.insert(-1, (3, 5 + 2 * (k - 1), "MLP: gather barrier -> last layer barrier"))
    got = {(wg, name): [] for wg in (0, 1) for _, _, name in table}
    for _ in range(args.reps):
        buf.zero_()
        torch.cuda.synchronize()
        lib.gnf_trace_set_buffer(C.c_void_p(buf.data_ptr()), launches)   # (the launch counter restarts: one slot per launch of the step)
        forward_shard_sums(net, graph)
        torch.cuda.synchronize()
        t = buf.cpu()
        assert int((t[:, :, :, END] != 0).sum()) == launches * 2 * WAVES, "a step is 2 T launches of k_half_fused_geo, every wave stamped"
        for wg in (0, 1):
            for a, b, name in table:
                d = (t[:, wg, :, b] - t[:, wg, :, a]).double().mean(dim=1)   # per launch: mean over the 8 waves
                got[(wg, name)] += d.tolist()
    lib.gnf_trace_set_buffer(None, 0)
    print(f"# instance: {'one net per wave, a barrier per layer (force_shape = 13)' if args.parent else 'both nets per wave, a barrier inside each phase (automatic dispatch)'}")
    print(f"# k_half_fused_geo phase table, workload {args.workload}: {n_global} nodes, {launches} launches per step, {args.reps} steps; shader cycles")
    print("# (mean over the 8 waves of a workgroup, median / min / max over launches and steps; stamped build)")
    print(f"# {'phase':46s} {'workgroup 0':>26s} {'mid-grid workgroup':>26s}")
    for _, _, name in table:
        cells = []
        for wg in (0, 1):
            v = got[(wg, name)]
            cells.append(f"{statistics.median(v):9.0f} [{min(v):7.0f},{max(v):7.0f}]")
        print(f"  {name:46s} {cells[0]:>26s} {cells[1]:>26s}")


if __name__ == "__main__":
    main()
