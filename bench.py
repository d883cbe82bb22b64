#!/usr/bin/env python3
"""bench.py -- chirp frames/s of the receiver's per-frame DSP on MI355X.

One "step" = one pass of the hot path (uc_process_batch, variant RX_REAL:
ingest -> window*chirp -> 2048-pt FFT -> windowed peak pick -> up/down symbol)
over one batch of synthetic frames already resident in HBM.

  N = 1   BASELINE.json configs[1]: 1 Mi x 2048-sample fp32 frames, random orthogonal up/down
          chirps at -10 dB SNR, literal TIME_FRAME (the firmware's reference tables).
  N > 1   BASELINE.json configs[4]: the frame index space is block-partitioned (weak scaling:
          1 Mi frames per GPU, no data-path collective); the frames are the K7 wire format
          (G, 7 x H, L, 96 data bits of "Hello World!", 12 x G) repeated over the GLOBAL frame
          index at -10 dB, reference sweep matched to the frame; the decoded symbol stream
          (1 B/frame) is all-gathered over RCCL every step inside the timed region (the gather of
          step k overlaps the kernel of step k + 1) and decoded to text after it.

`python bench.py --gpus N` starts its N ranks itself (one process per GPU, before anything touches
the GPU); under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` it is
one of the ranks.  --gpus must equal the world size.  Prints ONE JSON line on rank 0.

A plain N = 1 run sets up, warms up, times --steps steps and prints the contract line (metric, value, unit, higher_is_better,
dtype, ms_per_step, the configuration); --dump-outputs DIR writes the symbols of the last timed step as DIR/symbols.npy.
With --full the N = 1 line also carries (after the timed region, which they do not touch) the HIP-event kernel time and the
roofline (live clock, PMC traffic, achievable HBM, power), the bit error rate, cpu_baseline with the oracle gate, and:
  configs        BASELINE configs[2] (base-band I/Q, n = 1024, on the fs = 100 kHz pass-band stream; the firmware-window
                 mode beside it) and configs[3] (UC_STREAM, D = 8, replayed from a captured hipGraph; the eager rate
                 beside it), each with ms_per_step, kernel time by HIP events and both rooflines
  hello_world1   the N > 1 leg (configs[4]: K7 framing, RCCL all-gather every step, decode) at world size 1: the
                 like-for-like anchor of the driver's 1 -> N scaling efficiency
  roofline.valu  VALU issue fraction from the committed counter passes (profiles/r*_valu_insts.json); `bound` names the
                 larger of the HBM and the VALU fraction
Exit status: 3 if a correctness gate fails (symbols differ from the oracle on clear frames, a transmission does not
decode, the gathered stream is inconsistent) -- the JSON line is still printed.

Never run `--gpus N > 1` under rocprofv3: the profiler initialises the GPU in this parent, which then starts N children.
Profile one rank instead (RANK=0 WORLD_SIZE=1 ... rocprofv3 ... -- python3 bench.py), see tools/profile_round.sh.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "ultrasonic-communication_amd"))

# (round 6: the measuring helpers and the side legs live in modules of their own; this file keeps the contract: arguments, the
# ranks, the timed region, the JSON line)
from bench_telemetry import *  # noqa: E402,F401,F403
from bench_legs import *  # noqa: E402,F401,F403


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1 << 20, help="frames per GPU per step")
    ap.add_argument("--snr", type=float, default=-10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--ramp-ms", type=float, default=150.0,
                    help="untimed kernel launches before the warm-up steps until the GPU's clocks have settled (0 = none)")
    ap.add_argument("--variant", default="rx_real",
                    choices=["rx_real", "sync_cplx", "compress", "dechirp_down", "iq", "iq1024", "iq_bb", "iq1024_bb", "stream"],
                    help="default rx_real = BASELINE configs[1]; the others are side measurements")
    ap.add_argument("--no-configs", action="store_true", help="N = 1: skip the configs[2] / configs[3] block")
    ap.add_argument("--no-hello1", action="store_true", help="N = 1: skip the configs[4] leg at world size 1")
    ap.add_argument("--no-receive", action="store_true", help="N = 1: skip the multi-stream receiver leg")
    ap.add_argument("--sustain-s", type=float, default=1.5,
                    help="N = 1: seconds of untimed back-to-back launches behind the timed region during which socket power and "
                         "the SMU clock are sampled (hwmon); 0 = none")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="N = 1: do not run the two rocprofv3 --pmc child passes (FETCH_SIZE, WRITE_SIZE); roofline.traffic then "
                         "comes from the committed record and says so")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="N > 1: weak (default, the contract's line) = --frames per GPU; strong = --frames IN ALL, uc_partition shares "
                         "of --frames / N per GPU (N must divide it), the same gather -- the launch, tail and gather costs that a "
                         "fixed 1 Mi frames per GPU hides show here")
    ap.add_argument("--single-process", action="store_true",
                    help="--gpus N in ONE process: a uc_group over N devices (include/uchirp.h), as a C host would drive the node "
                         "(tests/c/host_multi.c); the default is one process per GPU")
    ap.add_argument("--full", action="store_true",
                    help="N = 1: also run everything beside the headline behind the timed region -- roofline (HIP-event kernel "
                         "time, live clock, PMC traffic, achievable HBM), power, configs[2] / configs[3], hello_world1, receive, "
                         "cpu_baseline -- and their gates; a plain run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (the arrays its caller receives) as "
                         "DIR/<name>.npy in float32; above %d MB in all, a fixed seeded sample of their rows" % (DUMP_BYTES // 10**6))
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


class Watchdog:
    """A rank that hangs (a peer died inside a collective, a rendezvous that never completes) must end the run LOUDLY and
    soon, not sit until the driver's own limit kills it without a line of output.  Every rank starts one: the main thread
    marks its progress (`mark`), a daemon thread checks the clock; past the limit it prints which rank, in which phase, after
    which step, for how long -- and ends the process with status 4 (os._exit: a thread cannot unblock a collective; the
    launcher then ends the other ranks).  UC_BENCH_TIMEOUT seconds WITHOUT PROGRESS (default 300: no phase of a healthy run --
    the first `import torch` on a fresh box, the rendezvous, a timed step -- takes that long; a slow but healthy 8-rank run
    keeps marking progress and is not cut off) and three times that for the whole run; never a retry."""

    def __init__(self, rank, world, limit_s):
        import threading
        self.rank, self.world, self.limit = rank, world, float(limit_s)
        self.t0 = time.time()
        self.phase, self.step, self.t_mark = "start", -1, self.t0
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)
        self._th.start()

    def mark(self, phase, step=-1):
        self.phase, self.step, self.t_mark = phase, step, time.time()

    def stop(self):
        self._stop.set()

    def _run(self):
        while not self._stop.wait(0.5):
            now = time.time()
            if now - self.t_mark > self.limit or now - self.t0 > 3.0 * self.limit:
                sys.stderr.write("bench.py WATCHDOG: rank %d of %d gave up after %.0f s (UC_BENCH_TIMEOUT): last progress %.1f s ago, "
                                 "phase '%s'%s -- a peer has probably died or never arrived; exiting with status 4\n"
                                 % (self.rank, self.world, now - self.t0, now - self.t_mark, self.phase,
                                    (", last completed step %d" % self.step) if self.step >= 0 else ""))
                sys.stderr.flush()
                os._exit(4)


def shard_frames(args, world):
    """frames per GPU and step: --frames (weak scaling, the contract's line) or --frames / world (strong: --frames in all, the
    equal uc_partition shares)"""
    if args.scaling == "strong" and world > 1:
        if args.frames % world:
            raise SystemExit("bench.py --scaling strong: %d GPUs do not divide %d frames" % (world, args.frames))
        return args.frames // world
    return args.frames


def bench_timeout():
    return float(os.environ.get("UC_BENCH_TIMEOUT", "300"))


def launch_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start the N ranks as fresh child processes.
    This parent never imports torch and never touches the GPU (a process that has initialised the GPU
    must not be replaced or forked on this pool); it relays rank 0's JSON line and the worst exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    import tempfile
    out0 = tempfile.TemporaryFile()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        # This pool's host driver only supports dmabuf IPC: without HSA_ENABLE_IPC_MODE_LEGACY=0 RCCL's intra-node setup
        # (hipIpcGetMemHandle) fails with "invalid argument".  The image exports it already; keep it if a caller's
        # environment dropped it.  (setdefault: an explicit value from the caller wins.)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("NCCL_DEBUG", "WARN")         # a failing RCCL call says why, on stderr, in the run that failed
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else sys.stderr))
    # every rank carries a watchdog of its own (UC_BENCH_TIMEOUT: 300 s without progress, 900 s in all) and reports where it hung;
    # this parent waits a little longer than the ranks' own cap, then says which ranks were still alive and ends exactly those
    deadline = time.time() + 3.0 * bench_timeout() + 15.0
    rc = 0
    while rc == 0 and any(p.poll() is None for p in procs):
        time.sleep(0.2)
        rc = next((p.returncode for p in procs if p.poll() not in (None, 0)), 0)
        if time.time() > deadline:
            rc = -1
    if rc:
        alive = [r for r, p in enumerate(procs) if p.poll() is None]
        ended = {r: p.returncode for r, p in enumerate(procs) if p.poll() is not None}
        sys.stderr.write("bench.py: %s; ranks still running: %s; ranks that had ended (exit status): %s -- ending the rest\n"
                         % ("timed out" if rc == -1 else "a rank failed (exit %s)" % rc, alive, ended))
        for p in procs:                      # a rank died or hung: the others wait in a collective; end exactly those
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    out0.seek(0)
    text = out0.read().decode()
    # stdout carries the JSON line(s) only; anything a library printed on rank 0's stdout goes to stderr.  Exit status 3
    # = a correctness gate failed on rank 0: its JSON line (with `gates_failed`) is still relayed.
    for ln in text.splitlines():
        (sys.stdout if ln.startswith("{") and rc in (0, 3) else sys.stderr).write(ln + "\n")
    sys.stdout.flush()
    if rc:
        raise SystemExit("bench.py: a rank failed (exit %s)" % rc if rc != 3 else 3)


def single_process(args):
    """`python bench.py --gpus N --single-process`: configs[4] with ONE host process driving all N GPUs through a uc_group
    (include/uchirp.h: uc_group_create = ncclCommInitAll, one launch stream + one gather stream per device) -- the shape a C
    host of the library has (tests/c/host_multi.c is that host in C99); same workload, same timed region, same JSON line as
    the one-process-per-GPU run.  torch only makes the frames and holds the buffers."""
    import hashlib
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    world = args.gpus
    # UC_BENCH_REHEARSE=1 (with UC_TUNING=1 UC_GROUP_SHARE_DEVICES=1 UC_RCCL_LIB=<tests/stubs/loopback_rccl.cpp built>): every
    # rank on device 0, the loop-back stand-in for RCCL -- the plumbing of this mode on a one-GPU box, never a measurement
    rehearse = os.environ.get("UC_BENCH_REHEARSE") == "1"
    if not rehearse and torch.cuda.device_count() < world:
        raise SystemExit("bench.py --single-process --gpus %d: only %d device(s) visible" % (world, torch.cuda.device_count()))
    import uchirp
    from uchirp import synth
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)                              # RCCL's banner and anything else on descriptor 1 goes to stderr
    nf, mag_mean = shard_frames(args, world), 1000.0
    devs = [torch.device("cuda", 0 if rehearse else d) for d in range(world)]
    wd = Watchdog(0, 1, bench_timeout())      # (one process: ncclCommInitAll and the in-process gathers can hang too)
    wd.mark("uc_group_create (ncclCommInitAll over %d devices)" % world)
    grp = uchirp.Group(uchirp.RX_REAL, devices=[d.index for d in devs], mag_mean=mag_mean, time_frame=MATCHED_TIME_FRAME)
    frames, streams = [], []
    for r, d in enumerate(devs):
        f, _ = synth.device_hello_frames(r * nf, nf, d, seed=1234 + r, snr_db=args.snr, msg=MSG)
        frames.append(f)
        streams.append(torch.cuda.Stream(d))
    gat = [[torch.empty(world * nf, dtype=torch.uint8, device=d) for d in devs] for _ in range(NBUF)]
    handles = [st.cuda_stream for st in streams]

    def step(k, ev=None):
        if ev is not None:
            for r in range(world):
                if k >= NBUF:                 # the write-after-gather wait in FRONT of the bracket: [e0, e1] = the kernel alone
                    grp.wait_gather(r, gat[k % NBUF][r], handles[r])
                ev[r][0].record(streams[r])
        grp.process(frames, world * nf, gat[k % NBUF], streams=handles)
        if ev is not None:
            for r in range(world):
                ev[r][1].record(streams[r])

    def sync():
        grp.synchronize()
        for d in devs:
            torch.cuda.synchronize(d)

    ramp_launches = 0
    t_r = time.perf_counter()
    while args.ramp_ms > 0 and (time.perf_counter() - t_r) * 1e3 < args.ramp_ms:
        for _ in range(4):
            step(0)
        sync()
        ramp_launches += 4
    wd.mark("warm-up")
    for k in range(args.warmup):
        step(k)
        wd.mark("warm-up", k)
    sync()
    evs = []
    for k in range(args.steps):
        row = []
        for d in devs:
            with torch.cuda.device(d):
                row.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        evs.append(row)
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, evs[k])
        wd.mark("timed region: enqueued", k)
    wd.mark("timed region: waiting for the devices (gathers included)", args.steps - 1)
    sync()
    elapsed = time.perf_counter() - t0
    wd.stop()
    km = np.array([[a.elapsed_time(b) for a, b in row] for row in evs]).mean(axis=0)       # kernel ms by device
    last = gat[(args.steps - 1) % NBUF]
    host = [g.cpu().numpy() for g in last]
    if args.dump_outputs:                     # the gathered symbol stream (every device holds it: digests below)
        dump_outputs(args.dump_outputs, {"symbols": host[0]})
    digs = [hashlib.sha256(h.tobytes()).hexdigest() for h in host]
    gate_failures = []
    if len(set(digs)) != 1:
        gate_failures.append("devices hold different gathered symbol streams")
    texts = synth.decode_hello(host[0], len(MSG))
    good = sum(1 for t in texts if t == MSG)
    if good != len(texts):
        gate_failures.append("hello: %d of %d transmissions decode" % (good, len(texts)))
    data = synth.hello_kind_stream(0, world * nf, MSG)
    m = data != 2
    value = world * nf * args.steps / elapsed
    out = {"metric": "chirp frames/s (2048-pt FFT demod)", "value": value, "unit": "frames/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
           "scaling": args.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "ramp_ms": args.ramp_ms,
           "ramp_launches": ramp_launches,
           "gather_backend": "uc_group_process_batch in ONE process: ncclCommInitAll, ncclAllGather in place per device inside "
                             "one ncclGroupStart/End, called from C",
           "config": {"workload": "configs[4]: %d x 2048-sample fp32 frames per GPU, frame-sharded 'Hello World!' stream (K7 "
                                  "framing repeated over the global frame index), SNR %.0f dB, rx_real with the reference "
                                  "sweep matched to the frame" % (nf, args.snr),
                      "frames_per_gpu": nf, "frame_len": N, "variant": "rx_real", "time_frame": MATCHED_TIME_FRAME,
                      "parallelism": "frame-sharded x%d, ONE host process (uc_group), RCCL all-gather of the symbol stream "
                                     "(1 B/frame) every step" % world},
           "roofline": roofline("band_rx_real_f32", "band_kernel<rx_real,f32>", nf, BYTES_PER_FRAME, float(km.max())),
           "per_rank": {"kernel_ms_by_rank": [float(v) for v in km]},
           "gather_ms_exposed": elapsed / args.steps * 1e3 - float(km.max()),
           "value_per_gpu": value / world, "symbols_sha256": digs[0],
           "decoded_text_first": texts[0] if texts else "", "transmissions": len(texts),
           "transmissions_decoded_exactly": good,
           "bit_error_rate_vs_transmitted": float((host[0][m] != data[m]).mean()),
           "gates_failed": gate_failures}
    if rehearse:
        out["rehearsal"] = "every rank on device 0, loop-back stand-in for RCCL: plumbing only, not a measurement"
    print(json.dumps(out), file=json_out, flush=True)
    grp.close()
    if gate_failures:
        sys.stderr.write("bench.py: correctness gate(s) failed: %s\n" % "; ".join(gate_failures))
        raise SystemExit(3)


def main():
    args = parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if args.single_process and env_world is None:
        return single_process(args)
    if env_world is None and args.gpus > 1:
        return launch_ranks(args)
    world = int(env_world or "1")
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d. Run `python bench.py --gpus N` (it starts its own ranks) "
                         "or `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`."
                         % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    # UC_BENCH_REHEARSE=1: plumbing rehearsal of the N > 1 path (spawn, rendezvous, symbol gather, concatenation
    # check, text decode, JSON line) with gloo.  On a ONE-GPU box every rank runs the real kernel on device 0; on a
    # box without a GPU NO kernel runs (the "decoded" symbols are the transmitted ones) and `value` is null.
    # Never a measurement.
    rehearse = os.environ.get("UC_BENCH_REHEARSE") == "1"
    have_gpu = torch.cuda.is_available()
    if not have_gpu and not rehearse:
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if rehearse:
        local_rank = 0
    device = torch.device("cuda", local_rank) if have_gpu else torch.device("cpu")
    if have_gpu:
        torch.cuda.set_device(local_rank)
    dist = None
    wd = Watchdog(rank, world, bench_timeout() if world > 1 else 1e9)
    # UC_BENCH_HELLO=1: run the N > 1 leg -- configs[4] framing, RCCL process group, async all-gather, digest check,
    # text decode -- with whatever world size there is, 1 included (what a one-GPU box can exercise of it on RCCL).
    multi = world > 1 or os.environ.get("UC_BENCH_HELLO") == "1"
    # RCCL prints its version banner on file descriptor 1 (the N = 1 run starts it too, for `hello_world1`); stdout must
    # carry the JSON line and nothing else: keep a private copy of the real stdout for that line and point descriptor 1
    # at stderr for everyone else
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:      # (UC_BENCH_HELLO=1 outside a launcher: one process, any free port)
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        os.environ.setdefault("NCCL_DEBUG", "WARN")  # (also under torch.distributed.run: RCCL's own reason for a failure, on stderr)
        wd.mark("rendezvous (torch.distributed.init_process_group)")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        world = dist.get_world_size()          # n_gpus printed below is what the process group reports
        wd.mark("rendezvous done")

    from uchirp import synth
    mag_mean = 1000.0
    nf = shard_frames(args, world)
    hello = multi and args.variant == "rx_real"
    eng = None
    if have_gpu:
        import uchirp
        vmap = {"rx_real": (uchirp.RX_REAL, {}), "sync_cplx": (uchirp.SYNC_CPLX, {}), "compress": (uchirp.COMPRESS, {}),
                "dechirp_down": (uchirp.DECHIRP_DOWN, {}), "iq": (uchirp.IQ, {}), "iq1024": (uchirp.IQ, {"n": 1024}),
                "stream": (uchirp.STREAM, {})}
        for nn in (2048, 1024):   # base-band I/Q, configs[2]'s constants (the batch is not its workload: timing only)
            vmap["iq_bb" if nn == 2048 else "iq1024_bb"] = (uchirp.IQ, dict(
                n=nn, fs=100000.0, carrier=18000.0, f0=16500.0, f1=19500.0, time_frame=nn / 100000.0,
                flags=uchirp.FLAG_IQ_BASEBAND))
        vid, vkw = vmap[args.variant]
        if hello:
            vkw = dict(vkw, time_frame=MATCHED_TIME_FRAME)
        eng = uchirp.Engine(vid, device=local_rank, mag_mean=mag_mean, **vkw)
    # The gather of the N > 1 leg goes through the C-ABI: a uc_group of one rank per process (include/uchirp.h,
    # uc_group_create_rank) -- the RCCL communicator is made from C out of a unique id that rank 0 draws and
    # torch.distributed merely carries to the others; every step decodes straight into the rank's slice of the gathered
    # stream and ncclAllGather runs in place on the group's gather stream.  torch.distributed stays the launcher's
    # rendezvous, the barrier and the max-over-ranks of the contract.  If any rank cannot build its group every rank
    # falls back to torch.distributed's all_gather_into_tensor (recorded as `gather_backend`); UC_BENCH_TORCH_GATHER=1
    # selects that path outright.
    # (UC_BENCH_REHEARSE=1 on a one-GPU box: the group path runs too when the loop-back stand-in for RCCL is named --
    # UC_TUNING=1 UC_RCCL_LIB=<tests/stubs/loopback_rccl.cpp built> -- otherwise the rehearsal gathers through gloo)
    grp, gather_backend = None, "torch.distributed all_gather_into_tensor"
    if (multi and args.variant == "rx_real" and have_gpu and os.environ.get("UC_BENCH_TORCH_GATHER") != "1"
            and (not rehearse or os.environ.get("UC_RCCL_LIB"))):
        ctl = torch.device("cpu") if rehearse else device           # where the launcher's own collectives live (gloo / RCCL)
        idt = torch.zeros(uchirp.GROUP_ID_BYTES, dtype=torch.uint8, device=ctl)
        why = ""
        # Preflight on EVERY rank, agreed on before anybody enters ncclCommInitRank: a rank that cannot load RCCL, select its
        # device or make a context would never arrive there, and the others would wait for it until the watchdog fires.
        wd.mark("uc_group_preflight")
        pre = 1
        try:
            uchirp.Group.preflight(uchirp.RX_REAL, device=local_rank, mag_mean=mag_mean, time_frame=MATCHED_TIME_FRAME)
        except Exception as ex:
            pre, why = 0, "preflight on rank %d: %s" % (rank, ex)
        pf = torch.tensor([pre], dtype=torch.int32, device=ctl)
        dist.all_reduce(pf, op=dist.ReduceOp.MIN)
        pre_all = int(pf.item()) == 1
        if rank == 0 and pre_all:
            try:
                idt.copy_(torch.frombuffer(bytearray(uchirp.Group.unique_id()), dtype=torch.uint8))
            except Exception as ex:                      # (an all-zero id tells the others)
                why = str(ex)
        dist.broadcast(idt, 0)
        ok = 0
        wd.mark("uc_group_create_rank (ncclCommInitRank)")
        if pre_all and bool(idt.any().item()):
            try:
                grp = uchirp.Group(uchirp.RX_REAL, world=world, rank=rank, unique_id=idt.cpu().numpy().tobytes(),
                                   device=local_rank, mag_mean=mag_mean, time_frame=MATCHED_TIME_FRAME)
                ok = 1
            except Exception as ex:
                why = str(ex)
        flag = torch.tensor([ok], dtype=torch.int32, device=ctl)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 1:
            gather_backend = "uc_group_process_batch: RCCL (ncclAllGather, in place) called from C on the group's gather stream"
        else:
            if grp is not None:
                grp.close()
                grp = None
            gather_backend += " (uc_group unavailable: %s)" % (why[:200] or "another rank failed")
    if hello:
        # rank r owns frames [r nf, (r + 1) nf) of the global stream (uc_partition, equal shares)
        frames, sent = synth.device_hello_frames(rank * nf, nf, device, seed=1234 + rank, snr_db=args.snr, msg=MSG)
    else:
        frames, sent = synth.device_frames(nf, device, seed=1234 + rank, snr_db=args.snr)
    if args.variant != "rx_real":
        sys.stdout = json_out                  # (the side measurements print their line themselves)
        return side_measurement(args, eng, frames, world, rank, torch)
    # NBUF symbol buffers in rotation: the gather of step k (RCCL's own stream) overlaps the kernels of the steps behind it;
    # a buffer is rewritten only after the gather that read it has finished (work.wait() orders the
    # launch stream behind it without blocking the host).
    sym2 = [torch.empty(nf, dtype=torch.uint8, device=device) for _ in range(NBUF)]
    gathered2 = [torch.empty(world * nf, dtype=torch.uint8, device=device) for _ in range(NBUF)] if multi else None
    works = [None] * NBUF
    stream = torch.cuda.current_stream(device) if have_gpu else None
    # the group's launches go to a stream of their own (a NULL entry in uc_group_process_batch's stream list means "the
    # group's own stream", and torch's default stream IS the NULL stream: the HIP events must sit where the kernel runs)
    gstream = torch.cuda.Stream(device) if grp is not None else None

    def gather(b):
        if rehearse:  # gloo has no device all-gather: stage through the host (rehearsal only)
            host = [torch.empty(nf, dtype=torch.uint8) for _ in range(world)]
            dist.all_gather(host, sym2[b].cpu())
            gathered2[b].copy_(torch.cat(host))
            return None
        return dist.all_gather_into_tensor(gathered2[b], sym2[b], async_op=True)

    def step(k, e0=None, e1=None):
        b = k % NBUF
        if grp is not None:                   # decode into this rank's slice of gathered2[b] + in-place all-gather, all in C
            if e0 is not None:
                # the write-after-gather wait for the gather that last used this buffer goes in FRONT of e0 (the library
                # would enqueue the same wait behind it): [e0, e1] brackets the kernel alone, and what a step costs beyond
                # the kernel -- that wait included -- shows up in gather_ms_exposed, where it belongs
                if k >= NBUF:
                    grp.wait_gather(0, gathered2[b], gstream.cuda_stream)
                e0.record(gstream)
            grp.process([frames], world * nf, [gathered2[b]], streams=[gstream.cuda_stream])
            if e1 is not None:
                e1.record(gstream)
            return
        if works[b] is not None:
            works[b].wait()
            works[b] = None
        if eng is None:                       # rehearsal without a GPU: no kernel, the transmitted symbols
            sym2[b].copy_(torch.where(sent == 2, torch.full_like(sent, 0xFF), sent))
        else:
            if e0 is not None:
                e0.record(stream)
            eng.process(frames, want_stats=False, symbols_out=sym2[b], stream=stream.cuda_stream)
            if e1 is not None:
                e1.record(stream)
        if multi:
            works[b] = gather(b)

    def drain():
        if grp is not None:
            grp.synchronize()
        for b in range(NBUF):
            if works[b] is not None:
                works[b].wait()
                works[b] = None

    def sync():
        if have_gpu:
            torch.cuda.synchronize()

    # Clock ramp (untimed, BEFORE the W warm-up steps; --ramp-ms, default 150): an idle MI355X needs ~20 launches
    # (~40 ms) of this kernel before its launch time settles -- 2.9, 3.0, 2.7, 2.5 ms for the first four launches,
    # 2.22 ms for launches 5-14, 2.10 ms from launch 20 on (tools/ramp_probe.py, profiles/r02_v5_ramp.txt).  The ramp
    # runs the kernel only (no gather), on the same resident batch, and is reported as `ramp_ms` in the JSON line.
    ramp_launches = 0
    if have_gpu and args.ramp_ms > 0:
        t_r = time.perf_counter()
        while (time.perf_counter() - t_r) * 1e3 < args.ramp_ms:
            for _ in range(4):
                eng.process(frames, want_stats=False, symbols_out=sym2[0], stream=stream.cuda_stream)
            torch.cuda.synchronize()
            ramp_launches += 4
    wd.mark("warm-up")
    for k in range(args.warmup):
        step(k)
        wd.mark("warm-up", k)
    drain()
    sync()
    wd.mark("barrier in front of the timed region")
    if multi:
        dist.barrier()
    sync()

    # A plain N = 1 run does what its headline needs and no more; the rest of the line -- kernel time, roofline, power, the
    # side legs and their gates -- is --full's.  The N > 1 line keeps its per-rank figures and decode gates (its workload's).
    extra = args.full or multi
    # per-launch kernel time: HIP events on the stream the kernel is launched on
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if have_gpu and extra else (None, None)
          for _ in range(args.steps)]
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, ev[k][0], ev[k][1])
        wd.mark("timed region: enqueued", k)
    wd.mark("timed region: waiting for the device (gathers included)", args.steps - 1)
    drain()
    sync()
    wd.mark("barrier behind the timed region", args.steps - 1)
    if multi:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:       # what the caller of the last timed step holds: the (gathered) symbol stream
        last = (args.steps - 1) % NBUF
        dump_outputs(args.dump_outputs, {"symbols": gathered2[last] if multi else sym2[last]})
    wd.mark("checks behind the timed region", args.steps - 1)
    # Sustained run behind the timed region (untimed, N = 1 only): the SMU's power figure is a moving average over about a
    # second, so the 40 ms of the timed region cannot show it; 1.5 s of back-to-back launches can.  Reports the socket power
    # and the SMU's clock over the last 0.5 s, and the rate the kernel holds meanwhile.
    power_rec = None
    if eng is not None and not multi and rank == 0 and args.full and args.sustain_s > 0:
        power = PowerSampler(torch, device)
        power.start()
        t_s = time.perf_counter()
        n_s = 0
        while time.perf_counter() - t_s < args.sustain_s:
            for _ in range(16):
                eng.process(frames, want_stats=False, symbols_out=sym2[0], stream=stream.cuda_stream)
            torch.cuda.synchronize()
            n_s += 16
        t_e = time.perf_counter()
        power_rec = power.stop(t_e - 0.5, t_e)
        if power_rec:
            power_rec["sustained_frames_per_s"] = nf * n_s / (t_e - t_s)
            power_rec["sustained_s"] = t_e - t_s
    elapsed_local = elapsed
    if multi:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearse else device)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    symbols = sym2[(args.steps - 1) % NBUF]
    if grp is not None:                       # the kernel wrote this rank's symbols straight into its slice of the stream
        symbols = gathered2[(args.steps - 1) % NBUF][rank * nf:(rank + 1) * nf]
        if eng is not None:                   # the checker: the same shard through a plain context (uc_process_batch)
            eng.process(frames, want_stats=False, symbols_out=sym2[0], stream=stream.cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(symbols, sym2[0]), "the group's slice differs from uc_process_batch on the same shard"
    gathered_host = None
    if multi:
        # Every rank holds the concatenation of all ranks' symbols, rank order: its own slice equals what it
        # decoded, and every rank's gathered buffer has the same digest (so the other slices are the owners').
        import hashlib
        g = gathered2[(args.steps - 1) % NBUF]
        assert torch.equal(g[rank * nf:(rank + 1) * nf], symbols), "gathered symbol stream differs from this rank's symbols"
        gathered_host = g.cpu().numpy()
        dig = torch.frombuffer(bytearray(hashlib.sha256(gathered_host.tobytes()).digest()), dtype=torch.uint8).clone()
        digs = [torch.empty(32, dtype=torch.uint8) for _ in range(world)]
        if rehearse:
            dist.all_gather(digs, dig)
        else:
            dd = [torch.empty(32, dtype=torch.uint8, device=device) for _ in range(world)]
            dist.all_gather(dd, dig.to(device))
            digs = [d.cpu() for d in dd]
        assert all(torch.equal(d, digs[0]) for d in digs), "ranks hold different gathered symbol streams"
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) if have_gpu and extra else None
    # the clock the chip held under the kernel of the timed region, measured now, on this box (every rank: its own)
    clk_live = None
    if eng is not None and extra:
        clk_live = live_clock(eng, lambda: eng.process(frames, want_stats=False, symbols_out=sym2[0], stream=stream.cuda_stream))
    local_ms = elapsed_local / args.steps * 1e3
    per_rank = None
    if multi:
        # every rank's own kernel time and step time (not only rank 0's, not only the maximum): lets a reader of the
        # N > 1 line tell the gather's cost from a straggling rank
        mine = torch.tensor([kern_ms if kern_ms is not None else 0.0, local_ms], dtype=torch.float64,
                            device="cpu" if rehearse else device)
        alls = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(alls, mine)
        per_rank = np.array([a.cpu().numpy() for a in alls])       # [world, (kernel_ms, ms_per_step)]
        # who ran where: the device every rank holds (name, uuid, PCI bus id, LOCAL_RANK), the peer-access row the HIP runtime
        # reports from it to every visible device, and the clock its chip held -- so that a slow or mis-mapped rank of the first
        # real 8-GPU run can be named from the line alone
        topo = {"rank": rank, "local_rank": local_rank, "pid": os.getpid()}
        if have_gpu:
            try:
                pr = torch.cuda.get_device_properties(device)
                topo.update({"device": pr.name, "uuid": str(getattr(pr, "uuid", "")), "pci_bus_id": getattr(pr, "pci_bus_id", None),
                             "multi_processor_count": pr.multi_processor_count,
                             "can_access_peer": [bool(d == device.index or torch.cuda.can_device_access_peer(device.index, d))
                                                 for d in range(torch.cuda.device_count())],
                             "shader_clock_GHz_under_the_kernel": clk_live})
            except Exception as ex:             # (diagnostics must never fail the run)
                topo["error"] = str(ex)[:200]
        topo_all = [None] * world
        dist.all_gather_object(topo_all, topo)

    gate_failures = []
    if rank == 0:
        total_frames = world * nf * args.steps
        value = total_frames / elapsed
        out = {
            "metric": "chirp frames/s (2048-pt FFT demod)", "value": value if have_gpu else None, "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": args.scaling if world > 1 else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "ramp_ms": args.ramp_ms if have_gpu else 0.0, "ramp_launches": ramp_launches,
        }
        if multi:
            out["gather_backend"] = gather_backend
        if hello:
            out["config"] = {"workload": "configs[4]: %d x 2048-sample fp32 frames per GPU, frame-sharded 'Hello World!' "
                                         "stream (K7 framing: G, 7 H, L, 96 data bits, 12 G, repeated over the global frame "
                                         "index), SNR %.0f dB, rx_real with the reference sweep matched to the frame"
                                         % (nf, args.snr),
                             "frames_per_gpu": nf, "frame_len": N, "variant": "rx_real", "time_frame": MATCHED_TIME_FRAME,
                             "parallelism": "frame-sharded x%d, RCCL all-gather of the symbol stream (1 B/frame) every step"
                                            % world}
        else:
            out["config"] = {"workload": "configs[1]: %d x 2048-sample fp32 frames per GPU, orthogonal up/down-chirp "
                                         "symbol decision (rx_real), SNR %.0f dB" % (nf, args.snr),
                             "frames_per_gpu": nf, "frame_len": N, "variant": "rx_real",
                             "parallelism": "frame-sharded x%d, RCCL all-gather of symbols" % world}
        if have_gpu and extra:
            achieved = nf * BYTES_PER_FRAME / (kern_ms * 1e-3) / 1e9
            # HBM bytes per launch from the committed PMC passes (FETCH_SIZE x2 on gfx950 + WRITE_SIZE,
            # collected with rocprofv3 --pmc in their own runs: profiles/*_hbm_traffic.json), scaled to
            # this launch's frame count; null if no profile is committed.
            traffic, traffic_source = None, None
            try:
                import glob
                import re
                # the band kernel's own passes are named rNN_vM_hbm_traffic.json (other kernels carry their name)
                tf = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "*_hbm_traffic.json"))
                            if re.fullmatch(r"r\d+_v\d+_hbm_traffic\.json", os.path.basename(f)))[-1]
                traffic = json.load(open(tf))["hbm_bytes_per_frame"] * nf
                traffic_source = ("NOT measured in this run: FETCH_SIZE x 2 + WRITE_SIZE per frame of the committed "
                                  "rocprofv3 --pmc passes in %s, scaled to this launch's %d frames"
                                  % (os.path.relpath(tf, ROOT), nf))
            except Exception:
                traffic = None
            out["roofline"] = roofline("band_rx_real_f32", "band_kernel<rx_real,f32>", nf, BYTES_PER_FRAME, kern_ms,
                                       num_cus(torch, device), clk_live)
            out["roofline"]["bytes_per_frame"] = BYTES_PER_FRAME
            # socket power / cap / SMU clock over the last 0.5 s of a 1.5 s sustained run behind the timed region (null: multi-GPU
            # run, --sustain-s 0, or no hwmon access)
            out["roofline"]["power"] = power_rec
            if not multi and not args.no_live_traffic:
                t_c = time.perf_counter()
                lt = live_traffic()
                if lt:
                    traffic, traffic_source = lt["hbm_bytes_per_frame"] * nf, lt.pop("method")
                    lt["wall_s"] = time.perf_counter() - t_c
                    out["roofline"]["traffic_counters"] = lt
                    out["roofline"]["traffic_over_algorithmic"] = lt["hbm_bytes_per_frame"] / BYTES_PER_FRAME
            out["roofline"]["traffic"] = traffic
            out["roofline"]["traffic_source"] = traffic_source
            if not multi:
                ach = achievable_hbm(frames, stream, torch)
                if ach:
                    out["roofline"]["achievable"] = ach
                    out["roofline"]["frac_of_achievable_read"] = achieved / ach["read_stream_GBs"]
        if hello:
            # config 5 gate: the gathered stream decodes to the transmitted text
            texts = synth.decode_hello(gathered_host, len(MSG))
            good = sum(1 for t in texts if t == MSG)
            out["decoded_text_first"] = texts[0] if texts else ""
            out["transmissions"] = len(texts)
            out["transmissions_decoded_exactly"] = good
            data = synth.hello_kind_stream(0, world * nf, MSG)
            m = data != 2
            out["bit_error_rate_vs_transmitted"] = float((gathered_host[m] != data[m]).mean())
            if not have_gpu:
                out["rehearsal"] = "plumbing only: no GPU, no kernel ran, value is null"
            elif rehearse:
                out["rehearsal"] = "every rank on device 0, gloo: not a measurement"
            if good != len(texts):
                gate_failures.append("hello: %d of %d transmissions decode" % (good, len(texts)))
            out["value_per_gpu"] = value / world if have_gpu else None
            km, sm = per_rank[:, 0], per_rank[:, 1]
            out["per_rank"] = {"kernel_ms": {"min": float(km.min()), "median": float(np.median(km)), "max": float(km.max())},
                               "ms_per_step": {"min": float(sm.min()), "median": float(np.median(sm)), "max": float(sm.max())},
                               "kernel_ms_by_rank": [float(v) for v in km]}
            # what a step costs beyond the kernel on the slowest rank: the gather that the next kernel does not hide,
            # launch gaps, and (N > 1) waiting for the slowest rank inside the collective
            out["kernel_ms_covers"] = ("[e0, e1] on the group's launch stream around uc_group_process_batch ALONE: the "
                                       "write-after-gather wait for the buffer's previous gather is enqueued in FRONT of e0 "
                                       "(uc_group_wait_gather) since round 5 -- not comparable with kernel_ms of rounds 1-4, "
                                       "which included it; gather_ms_exposed = ms_per_step - kernel_ms carries it now")
            out["per_rank"]["roofline_frac_by_rank"] = ([float(nf * BYTES_PER_FRAME / (v * 1e-3) / 1e9 / HBM_PEAK_GBS) if v > 0 else None
                                                         for v in km] if have_gpu else None)
            out["per_rank"]["ranks"] = topo_all
            out["gather_ms_exposed"] = float((sm - km).max()) if have_gpu else None
            out["gather_ms_exposed_by_rank"] = [float(v) for v in (sm - km)] if have_gpu else None
            # the world size the C group's RCCL communicator reports (n_gpus above is torch.distributed's)
            out["rccl_world"] = int(grp.world) if grp is not None else None
            out["scaling_note"] = ("no 1 -> 8 curve has been measured by the builder (one-GPU boxes only): the first real "
                                   "N > 1 numbers are the driver's")
        elif args.full:
            # correctness figure of the measured run: decoded symbols vs transmitted bits.  ~23 % is EXPECTED here:
            # configs[1] runs the firmware's literal TIME_FRAME = 0.0205 s reference tables against frames that
            # sweep over the whole 26.2 ms frame; GPU == oracle is the gate (below), the matched sweep is configs[4]
            out["bit_error_rate_vs_transmitted"] = float((symbols != sent).float().mean().item())
            out["bit_error_rate_note"] = ("expected ~0.23: literal TIME_FRAME reference (SURVEY Q4) vs full-frame sweeps; "
                                          "the oracle has the same errors (symbols_equal_oracle_head4096_clear)")
        if not multi and have_gpu and args.full and not args.no_configs:
            cfgs = {}
            for name, fn in (("configs[2]", lambda: config2_iq(args, device, stream, torch, mag_mean)),
                             ("configs[3]", lambda: config3_stream(args, frames, device, torch))):
                t_c = time.perf_counter()
                try:
                    cfgs[name] = fn()
                except Exception as ex:                      # the contract line must not die with a side leg
                    cfgs[name] = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
                    gate_failures.append("%s failed: %s" % (name, type(ex).__name__))
                cfgs[name]["wall_s"] = time.perf_counter() - t_c
            out["configs"] = cfgs
            c2, c3 = cfgs["configs[2]"], cfgs["configs[3]"]
            if not c2.get("baseband", {}).get("symbols_equal_oracle_head4096_clear", 1.0) >= 1.0:   # (NaN fails too)
                gate_failures.append("configs[2]: base-band symbols differ from the oracle on clear frames (or none is clear)")
            if c3.get("graph_equals_eager") is False:
                gate_failures.append("configs[3]: graph replay differs from the eager launch")
            if c3.get("head_rel_err_vs_oracle", 0.0) > 2e-5 or c3.get("head_peak_offsets_equal_oracle") is False:
                gate_failures.append("configs[3]: stream head differs from the oracle")
        if not multi and have_gpu and args.full and not args.no_hello1:
            t_c = time.perf_counter()
            try:
                h1 = hello_world1(args, device, torch, mag_mean)
                if h1["transmissions_decoded_exactly"] != h1["transmissions"] or not h1["gathered_equals_decoded"]:
                    gate_failures.append("hello_world1: %d of %d transmissions decode"
                                         % (h1["transmissions_decoded_exactly"], h1["transmissions"]))
                h1["over_configs1_value"] = h1["value"] / value
            except Exception as ex:
                h1 = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
                gate_failures.append("hello_world1 failed: %s" % type(ex).__name__)
            h1["wall_s"] = time.perf_counter() - t_c
            out["hello_world1"] = h1
            if "value" in h1:
                # The N > 1 lines of the scaling curve run configs[4] (K7 framing, matched sweep, gather every step); THIS line
                # runs configs[1] (no gather).  Like for like, the curve's N = 1 point is this one: value(N) / N / anchor.
                out["scale_anchor"] = {"workload": "configs[4] at world size 1 (the workload of the --gpus N > 1 lines)",
                                       "n_gpus": 1, "value": h1["value"], "unit": "frames/s", "ms_per_step": h1["ms_per_step"],
                                       "how": "UC_BENCH_HELLO=1 python bench.py prints this leg as its contract line"}
        if not multi and have_gpu and args.full and not args.no_receive:
            t_c = time.perf_counter()
            try:
                rx = receive_leg(args, device, torch)
                for key in ("sync_cplx_4096_streams", "sync_cplx_64_streams", "sync_cplx_1_stream"):
                    if rx[key]["streams_decoding_the_text"] != rx[key]["streams"]:
                        gate_failures.append("receive: %d of %d streams decode the text"
                                             % (rx[key]["streams_decoding_the_text"], rx[key]["streams"]))
                if rx["live_4096_streams"]["streams_whose_chunks_add_up_to_the_recorded_call"] != 4096:
                    gate_failures.append("receive: live chunks differ from the recorded-stream call on %d streams"
                                         % (4096 - rx["live_4096_streams"]["streams_whose_chunks_add_up_to_the_recorded_call"]))
            except Exception as ex:
                rx = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:300])}
                gate_failures.append("receive failed: %s" % type(ex).__name__)
            rx["wall_s"] = time.perf_counter() - t_c
            out["receive"] = rx
        if not multi and have_gpu and args.full and not args.no_cpu_baseline:
            cb = cpu_baseline(frames[: 1 << 19].cpu().numpy(), mag_mean)
            # the oracle as the checker: GPU symbols of the measured run vs float64 oracle
            head, clear = cb.pop("symbols_f64_oracle_head"), cb.pop("clear_head")
            got = symbols[:4096].cpu().numpy()
            out["symbols_equal_oracle_head4096"] = float((got == head).mean())
            out["symbols_equal_oracle_head4096_clear"] = float((got[clear] == head[clear]).mean())
            if not np.array_equal(got[clear], head[clear]):
                gate_failures.append("configs[1]: symbols differ from the float64 oracle on clear frames")
            out["cpu_baseline"] = cb
        out["gates_failed"] = gate_failures
        print(json.dumps(out), file=json_out, flush=True)
    if grp is not None:
        grp.close()
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    if gate_failures:
        sys.stderr.write("bench.py: correctness gate(s) failed: %s\n" % "; ".join(gate_failures))
        raise SystemExit(3)


if __name__ == "__main__":
    main()
