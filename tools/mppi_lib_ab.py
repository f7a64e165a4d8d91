"""A-B of two builds of libtbnav_hip.so on the headline tick (K = 1024, T = 50, device noise): us per tick over 2000 ticks (graph replay)
and over 20-tick batches of plain launches (what the driver's --steps 20 times).  python tools/mppi_lib_ab.py <lib A> [lib B ...]
Each library is loaded in a process of its own.
  --dump DIR   no timing: every library writes DIR/<its position>/<shape>.npz instead — after three device-noise ticks (seed 42) the
               control sequence, the controls to apply, J of the last tick, and the K-slice records of a fourth tick — for (K, T) =
               (1024, 50), (1000, 50), (100, 50), (1024, 100), (2048, 30), (1024, 65), (2048, 50) and the arc dynamics at (1024, 50),
               (1024, 100), (1024, 65); the files of any two
               libraries are then compared array by array, bit for bit (exit code 1 on a difference)."""
import os, subprocess, sys, time
DUMP_SHAPES = [(1024, 50, "rk4"), (1000, 50, "rk4"), (100, 50, "rk4"), (1024, 100, "rk4"), (2048, 30, "rk4"), (1024, 50, "arc"),
               (1024, 100, "arc"), (1024, 65, "rk4"), (1024, 65, "arc"),   # (T = 65: two steps per lane, the last live lane half padding)
               (2048, 50, "rk4")]                                          # (the straight-line mppi_combine<4, 0> at the shipped horizon)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.load_package()
    from rtn_amd import capi
    if sys.argv[2] != "default":
        capi.LIB_PATH = os.path.abspath(sys.argv[2])
    import torch, bench
    if sys.argv[3:4] == ["--dump"]:
        import numpy as np
        from rtn_amd.mppi import MPPI, CartModel, LossFunc
        P = bench.SHIPPED
        os.makedirs(sys.argv[4], exist_ok=True)
        for K, T, dyn in DUMP_SHAPES:
            m = MPPI(CartModel(P["wheel_radius"], P["wheel_base"]), LossFunc(P["Q"], P["R"], P["P1"]), P["lam"], P["max_wheel_vel"], P["ul_var"],
                     P["ur_var"], (T + 0.5) * P["dt"], P["dt"], K, 0, keep_j=True)
            assert m.steps == T
            m.setWaypoint(*bench.WAYPOINT); m.setDynamics(dyn)
            x0 = (0.02, -0.01, 0.1)
            for tick in range(3):
                out = m.newControlsRng(x0, 42, tick)
            rec = torch.zeros(T, m.records_per_step, 8, dtype=torch.float64, device="cuda")
            u, J = m.getControls(), m.costToGo()
            m.shardPartialsRng(x0, 42, 3, rec.data_ptr()); torch.cuda.synchronize()
            np.savez(os.path.join(sys.argv[4], f"K{K}_T{T}_{dyn}.npz"), u=u, out=np.asarray(out), J=J, records=rec.cpu().numpy(),
                     kernels=np.asarray(m.lastKernelNames()))
            print(sys.argv[2], K, T, dyn, *m.lastKernelNames(), out, flush=True)
        sys.exit(0)
    m = bench.make_mppi(1024, 0.5, 0)
    torch.cuda.set_stream(torch.cuda.Stream())
    st = torch.cuda.current_stream().cuda_stream
    tk = 0
    def run(n):
        global tk
        m.enqueueRngBatch(bench.X0, 42, tk, n, st); tk += n
    run(300); torch.cuda.synchronize()
    res = []
    for rep in range(5):
        t0 = time.perf_counter(); run(2000); torch.cuda.synchronize(); long_us = (time.perf_counter() - t0) / 2000 * 1e6
        short = []
        for q in range(30):
            run(5); torch.cuda.synchronize()
            t0 = time.perf_counter(); run(20); torch.cuda.synchronize(); short.append((time.perf_counter() - t0) / 20 * 1e6)
        short.sort()
        res.append((long_us, short[len(short) // 2]))
    print(sys.argv[2], "us/tick over 2000 ticks:", " ".join(f"{a:.2f}" for a, _ in res), "| median of 20-tick batches:", " ".join(f"{b:.2f}" for _, b in res), flush=True)
    sys.exit(0)
args = sys.argv[1:]
dump = None
if "--dump" in args:
    i = args.index("--dump")
    dump = args[i + 1]
    del args[i:i + 2]
for n, lib in enumerate(args or ["default"]):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib] + (["--dump", os.path.join(dump, str(n))] if dump else []), check=False)
    if r.returncode != 0:   # (a child that faulted: nothing more is started on the device)
        sys.exit(f"{lib}: exit code {r.returncode}")
if dump:
    import numpy as np
    bad = 0
    for n in range(1, len(args)):
        for K, T, dyn in DUMP_SHAPES:
            a, b = (np.load(os.path.join(dump, str(q), f"K{K}_T{T}_{dyn}.npz")) for q in (0, n))
            for f in a.files:
                same = a[f].shape == b[f].shape and a[f].tobytes() == b[f].tobytes()
                bad += not same
                print(f"{args[n]} against {args[0]}: K={K} T={T} {dyn} {f}: {'identical' if same else 'DIFFERENT'}")
    sys.exit(1 if bad else 0)
