"""The path's program: what ``python rvap/vap_main/vap_main.py --vap_model ... --cpc_model ... --port_num_in 50007 --port_num_out 50008
--vap_process_rate 20 --context_len_sec 2.5 --gpu --audio_gain 1.0`` does (vap_main.py:461-530, and its bc / nod twins), for MANY dialogues and
MANY GPUs behind the reference's ONE port pair.  One process: one engine per GPU (``vapx_create`` with ``device_id = r``), one passive native
front-end per engine (its own receive / tick / send threads, ``vapx_ingest_*``), and one front door (``vapx_frontdoor_*``) that owns
``port_num_in`` / ``port_num_out`` and hands every accepted connection to a GPU.  Dialogue k lands on GPU ``k mod N`` (lowest free global slot) and
stays there — its state lives there; there is no collective.  Same argument names as the reference plus ``--streams`` (slots per GPU), ``--gpus``,
``--mode`` and ``--precision {auto,fp32,split}``.  ``auto`` (default) serves the arithmetic the load needs: fp32 — the reference's — while
``streams x frame rate`` keeps one GPU's fp32 path <= 85 % busy, the fp32-accurate split-precision engine beyond that, and it says so; when
NEITHER path holds the 10 ms bound at the requested ``--streams`` it refuses to start (``--allow-overload`` downgrades that to a warning).  The
rule and its measured rates: ``capacity.plan`` / DESIGN.md §5.

    python -m vap_realtime_amd.serve --vap_model asset/vap/vap_state_dict_jp_20hz_2500msec.pt --cpc_model asset/cpc/60k_epoch4-d0f474de.pt \\
        --streams 4096 --gpus 8

``--worker-procs`` (``auto`` turns it on when one process could not hold the descriptors: two sockets per dialogue against RLIMIT_NOFILE): the
front door becomes a process of its own that only accepts and routes, and every GPU gets a WORKER process — engine, front-end threads, sockets —
to which accepted connections are passed (``vapx_frontdoor_open_links`` / ``vapx_ingest_attach_link``, include/vapx.h).  Same ports, same
placement, same packets; 8 x 4096 dialogues need it in a container whose descriptor limit is 20 000.

``--mode a+b[+c]`` (distinct names from vap / bc / nod, the first leads) serves SEVERAL models on one shared CPC trunk — the reference's
``vap_main.py``, ``vap_bc_main.py`` and ``vap_nod_main.py`` side by side on one ``cpc_model`` file, with the audio encoded once: one input port, one
output port per model (``--port_num_out`` comma-separated, default 50008, 50009, ...), ``--vap_model`` one path per model, comma-separated in the
same order.  One GPU, one process: the front door and ``--worker-procs`` are single-model.  ``--vap_process_rate`` and
``--context_len_sec`` take one value per model, comma-separated in model order (a single value applies to all): the reference's own deployment
is ``--mode vap+bc+nod --vap_process_rate 20,20,10 --context_len_sec 2.5,5,10``.  The fastest model leads (ties: the first); a slower model's
rate must divide the leader's, and it answers every R-th input frame of a dialogue with one packet that echoes all R frames' samples, as its
reference program does.  ``--save_state`` / ``--load_state`` are refused for a group with a slower model (its half-collected frame is not
part of a snapshot yet).

``--load_state PATH`` / ``--save_state PATH`` keep the dialogues' state (LSTM, carry, context window, Q|K|V cache) across a restart: the
snapshot (``snapshot.py``) is imported after the engines are built and before the front-end opens, and written after the front-end has closed on
SIGTERM / SIGINT.  With ``--gpus N`` or worker processes every engine uses ``PATH.<rank>``; ``--mode a+b`` saves and loads the whole group.  A
missing ``--load_state`` file is a warning and a cold start; a file that does not fit the engines is refused at start-up (exit 1), never half-loaded.
An engine that loaded a snapshot opens its front-end without the warm-up on silence (done before the import instead) and WITHOUT reset-on-connect: a dialogue that (re)connects finds its slot's state — as in the
reference, which never resets the model on a reconnect and re-zeroes only the carry (vap_main.py:368-369) — where a cold engine starts every new
connection from a fresh stream.

``--synthetic-weights SEED`` serves seeded random weights (no checkpoint files: load tests, demos).  SIGTERM / SIGINT stop every GPU's
front-end and engine in order; a failure while one GPU comes up tears the others down and exits non-zero.
"""
from __future__ import annotations

import argparse
import json
import signal
import sys
import time


def load_blob(args):
    from . import checkpoints, weights as W
    if args.synthetic_weights is not None:
        cpc, vap = W.synthetic_weights(args.synthetic_weights, args.vap_process_rate, args.mode or "vap")
        return W.pack_blob(cpc, vap, args.mode or "vap"), args.mode or "vap"
    blob, hz, mode = checkpoints.import_checkpoints(args.vap_model, args.cpc_model, frame_rate=args.vap_process_rate, mode=args.mode)
    return blob, mode


def state_path(path, rank: int, n_engines: int, worker: bool = False):
    """The snapshot file of engine ``rank``: ``PATH`` for the one engine of a one-process service, ``PATH.<rank>`` with ``--gpus N`` or
    worker processes."""
    if not path:
        return None
    return f"{path}.{rank}" if (n_engines > 1 or worker) else path


def _warm_up(target):
    """What the front-end's open does for a cold engine (the first step of a process loads the code objects: hundreds of ms), done here
    because it must happen BEFORE a snapshot is imported: one tick of silence on max_batch streams, then those streams reset."""
    import numpy as np
    lead = target.leader if hasattr(target, "leader") else target
    if not hasattr(lead, "reset_stream"):
        return
    from . import pcm
    fmt = getattr(lead, "input_format", "f32")                                                   # --input_format: silence in that format
    silence = np.full((lead.max_batch, 2, getattr(lead, "hop_in", lead.hop)), pcm.SILENCE[fmt], pcm.DTYPES[fmt])      # hop_in: the hop at --input_rate
    if hasattr(target, "step_wire"):
        target.step_wire(silence)
    else:
        target.step(silence)
    for i in range(lead.max_batch):
        lead.reset_stream(i)


def load_state(path, target, tag: str = "") -> bool:
    """``--load_state``: False (and a warning) when there is no file — a cold start; True after an import; raises when the file does not
    fit ``target`` (nothing was imported then: snapshot.load validates first)."""
    import os
    from . import snapshot
    if not path:
        return False
    if not os.path.exists(path):
        print(f"[vapx] {tag}WARNING: --load_state {path}: no such file, cold start", file=sys.stderr, flush=True)
        return False
    _warm_up(target)                                             # before the import: the front-end will not step on silence over loaded state
    ids = snapshot.load(path, target)
    print(f"[vapx] {tag}state of {len(ids)} dialogue slot(s) loaded from {path}: connections keep their slot's state (no reset on connect)", flush=True)
    return True


def save_state(path, target, tag: str = "") -> bool:
    """``--save_state``: every slot, with the Q|K|V cache; call it once the front-end is closed (its tick thread is then stopped, so calls on
    the handle stay serialised).  A failure is reported, not raised: the shutdown goes on."""
    from . import snapshot
    if not path:
        return False
    try:
        hdr = snapshot.save(path, target)
    except Exception as e:                                      # noqa: BLE001
        print(f"[vapx] {tag}--save_state {path} failed: {e}", file=sys.stderr, flush=True)
        return False
    print(f"[vapx] {tag}state of {len(hdr['ids'])} dialogue slot(s) saved to {path}", flush=True)
    return True


def input_class_refusal(args, names=None):
    """Why ``--input_class`` cannot be served with the other options given, one line - or None.  ``names``: the models of ``--mode a+b``."""
    if not getattr(args, "input_class", None):
        return None
    if args.input_rate != 16000:
        return "--input_class with --input_rate: every class names its own rate (FORMAT@RATE)"
    if args.input_format != "f64":
        return "--input_class with --input_format: every class names its own format (FORMAT@RATE)"
    if names is not None:
        return f"--input_class with --mode {args.mode}: the group front-end has one input port, class ports serve one model"
    if args.gpus > 1 or args.worker_procs == "on" or args.worker_link is not None:
        return "--input_class with --gpus N > 1 (or worker processes): the front door has one input port, class ports serve one GPU"
    if args.load_state or args.save_state:
        return "--input_class with --save_state / --load_state: state records of an engine with input classes do not exist yet"
    return None


def rate_kw(args) -> dict:
    """``--input_rate`` and ``--input_format`` as ``Engine`` / ``TrunkGroup`` keywords; nothing at 16000 / f64, so such engines are built
    exactly as before.  The front-end reads both from the engine.  ``--input_class``: the table instead (``args.input_classes``)."""
    if getattr(args, "input_classes", None):
        return {"input_classes": args.input_classes}
    kw = {"input_hz": args.input_rate} if getattr(args, "input_rate", 16000) != 16000 else {}
    if getattr(args, "input_format", "f64") != "f64":
        kw["input_format"] = args.input_format
    return kw


def group_modes(mode):
    """``"bc+nod"`` -> ``["bc", "nod"]``; None for a single mode (or none).  Raises ValueError for unknown / repeated names."""
    if not mode or "+" not in mode:
        if mode and mode not in ("vap", "bc", "nod"):
            raise ValueError(f"--mode {mode}: choose from vap, bc, nod, or a+b[+c] of distinct ones")
        return None
    names = mode.split("+")
    if any(m not in ("vap", "bc", "nod") for m in names) or len(set(names)) != len(names):
        raise ValueError(f"--mode {mode}: a+b[+c] takes distinct names from vap, bc, nod")
    return names


def out_ports(args, n_models: int):
    """``--port_num_out``: one port per model, comma-separated (default 50008, 50009, ...)."""
    ports = [int(p) for p in str(args.port_num_out).split(",")]
    if len(ports) == 1 and n_models > 1 and args.port_num_out_default:
        ports = [ports[0] + i for i in range(n_models)]
    if len(ports) != n_models:
        raise ValueError(f"--port_num_out names {len(ports)} port(s) for {n_models} model(s)")
    return ports


def per_model(value, n_models: int, cast, flag: str):
    """``"20,20,10"`` -> ``[20, 20, 10]``; a single value applies to every model.  Raises ValueError for another count."""
    parts = [cast(p) for p in str(value).split(",")]
    if len(parts) == 1:
        return parts * n_models
    if len(parts) != n_models:
        raise ValueError(f"{flag} names {len(parts)} value(s) for {n_models} model(s): give one, or one per model in model order")
    return parts


def group_plan(args, names):
    """Per-model geometry of a ``+`` mode (``engine.trunk_plan``) from ``--vap_process_rate`` / ``--context_len_sec``; raises ValueError for
    rates a shared trunk cannot serve and for ``--save_state`` / ``--load_state`` with a model slower than its leader."""
    from . import engine
    rates = per_model(args.vap_process_rate, len(names), int, "--vap_process_rate")
    ctxs = per_model(args.context_len_sec, len(names), float, "--context_len_sec")
    try:
        plan = engine.trunk_plan(names, rates, ctxs)
    except engine.VapxError as e:
        raise ValueError(str(e)) from None
    slow = [m for m in names if plan["R"][m] > 1]
    if slow and (args.save_state or args.load_state):
        raise ValueError(f"--save_state / --load_state with {'+'.join(slow)} at 1/{plan['R'][slow[0]]} of the leader's rate: a snapshot does not carry "
                         f"a slower model's half-collected frame yet (vapx_export_streams refuses it); serve this group without them")
    if len({(plan["hz"][m], plan["T"][m]) for m in names}) > 1 and (args.save_state or args.load_state):
        raise ValueError("--save_state / --load_state with models of different windows: a snapshot file describes ONE rate and window for the "
                         "whole group (the engines' own vapx_export_streams / vapx_import_streams handle each window)")
    return plan


def load_group_blobs(args, names):
    """{mode: blob} of a ``+`` mode, each model at its own rate; every model on the SAME CPC weights (vapx_attach_trunk refuses otherwise)."""
    from . import checkpoints, weights as W
    hz = args.group_plan["hz"]
    blobs = {}
    if args.synthetic_weights is not None:
        for m in names:                              # one seed -> identical CPC tensors in every mode and at every rate, only the rest differs
            cpc, vap = W.synthetic_weights(args.synthetic_weights, hz[m], m)
            blobs[m] = W.pack_blob(cpc, vap, m)
        return blobs
    paths = args.vap_model.split(",")
    if len(paths) != len(names):
        raise ValueError(f"--vap_model names {len(paths)} file(s) for --mode {'+'.join(names)}: one per model, comma-separated, in that order")
    for m, path in zip(names, paths):
        blobs[m] = checkpoints.import_checkpoints(path, args.cpc_model, frame_rate=hz[m], mode=m)[0]
    return blobs


def build_group(args, names):
    """One trunk group + one group front-end on GPU 0: (group, server)."""
    from . import dist_util, engine, ingest
    blobs = load_group_blobs(args, names)
    ports = out_ports(args, len(names))
    args.precision_plan = None
    gp = args.group_plan
    choose_precision(args, "+".join(names), [(m, gp["hz"][m], gp["ctx"][m]) for m in gp["order"]])   # every model at its own rate and window
    grp = srv = None
    try:
        grp = engine.TrunkGroup(blobs, gp["hz"], gp["ctx"], max_streams=args.streams,
                                max_batch=min(args.streams, args.max_batch), device_id=0, groups=2, split_f16=(args.precision == "split"),
                                **rate_kw(args))
        warm = load_state(state_path(args.load_state, 0, 1), grp)
        cores = None
        if args.pin:
            cores, _ = dist_util.front_end_placement(0, 1 + args.rx_threads + args.tx_threads)
        srv = ingest.NativeServer.for_group(grp, port_in=args.port_num_in, ports_out=ports, gain=args.audio_gain,
                                            max_wait_s=args.max_wait_ms * 1e-3, bind_any=args.bind_any, rx_threads=args.rx_threads,
                                            tx_threads=args.tx_threads, cores=cores, reset_on_connect=not warm, keep_state=warm)
    except Exception:
        if srv is not None:
            srv.close()
        if grp is not None:
            grp.close()
        raise
    return grp, srv


def run_group(args, names, stop) -> int:
    try:
        grp, srv = build_group(args, names)
    except Exception as e:                                      # noqa: BLE001
        print(f"[vapx] start-up failed: {e}", file=sys.stderr, flush=True)
        return 1
    outs = ", ".join(f"{m} :{srv.ports_out[m]}" for m in names)
    geo = ", ".join(f"{m} {grp.hz[m]} Hz / {grp.ctx[m]:g} s" for m in names)
    print(f"[vapx] 1 GPU(s) x {args.streams} dialogue slots, modes {'+'.join(names)} on one CPC trunk ({grp.order[0]} leads), {args.precision} "
          f"arithmetic, {geo}, audio at {args.input_rate} Hz ({args.input_format}) — input :{srv.port_in}, output {outs}", flush=True)
    last = time.time()
    while not stop["now"]:
        time.sleep(0.2)
        if args.stats_sec > 0 and time.time() - last >= args.stats_sec:
            last = time.time()
            st = srv.stats(reset_latency_window=True)
            print("[vapx] GPU 0: " + json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}), flush=True)
    srv.close()
    save_state(state_path(args.save_state, 0, 1), grp)
    grp.close()
    return 0


def choose_precision(args, mode, models=None):
    """``models``: [(mode, frame_hz, ctx_sec), ...] of a trunk group, leader first — each is priced at its own rate and window."""
    if args.precision == "auto":                 # serve the arithmetic the load needs (capacity.plan: measured sustained rate per path)
        from . import capacity
        pl = (capacity.plan_mixed(args.streams, models) if models else
              capacity.plan(args.streams, args.vap_process_rate, args.context_len_sec, mode))
        args.precision_plan = pl
        print(f"[vapx] --precision auto -> {pl['precision']}: {pl['reason']}", file=sys.stderr, flush=True)
        if not pl["ok"]:
            if not args.allow_overload:
                raise RuntimeError(pl["reason"] + " (start anyway with --allow-overload, or name a --precision)")
            print("[vapx] WARNING: starting overloaded (--allow-overload): frames WILL be answered later than 10 ms at full occupancy", file=sys.stderr, flush=True)
        args.precision = pl["precision"]


def wants_worker_procs(args) -> bool:
    """``--worker-procs auto``: a process per GPU when ONE process could not hold the sockets (2 per dialogue + slack) under RLIMIT_NOFILE."""
    if args.worker_procs != "auto":
        return args.worker_procs == "on"
    import resource
    hard = resource.getrlimit(resource.RLIMIT_NOFILE)[1]
    need = 2 * max(1, args.gpus) * args.streams + 256
    return args.gpus > 1 and hard != resource.RLIM_INFINITY and need > hard


def build(args):
    """(engines, shards, front door or None): N = 1 listens directly (no extra hop), N > 1 goes through the front door."""
    from . import dist_util, engine, ingest
    blob, mode = load_blob(args)
    n = max(1, args.gpus)
    args.precision_plan = None
    choose_precision(args, mode)
    engines, shards, door = [], [], None
    taken = {}                                   # cores of a NUMA node's run already given to an earlier shard's front-end
    try:
        for r in range(n):
            dev = 0 if args.share_gpu else r
            eng = engine.Engine(blob, args.vap_process_rate, args.context_len_sec, max_streams=args.streams,
                                max_batch=min(args.streams, args.max_batch), mode=mode, device_id=dev,
                                groups=2,   # two intra-tick overlap groups: ragged ticks of a few hundred streams get 20 % shorter
                                split_f16=(args.precision == "split"), **rate_kw(args))
            engines.append(eng)
            warm = load_state(state_path(args.load_state, r, n), eng, f"GPU {r}: ")
            passive = n > 1
            cores = None
            if args.pin:                  # tick / receive / sender threads next to their GPU, every shard on cores of its own
                node_key = tuple(dist_util.gpu_node_cores(dev)[:1])
                nthr = 1 + args.rx_threads + args.tx_threads
                cores, _ = dist_util.front_end_placement(dev, nthr, skip=taken.get(node_key, 0))
                taken[node_key] = taken.get(node_key, 0) + nthr
            shards.append(ingest.NativeServer(eng, port_in=-1 if passive else args.port_num_in, port_out=-1 if passive else args.port_num_out,
                                              gain=args.audio_gain, max_wait_s=args.max_wait_ms * 1e-3, bind_any=args.bind_any,
                                              rx_threads=args.rx_threads, tx_threads=args.tx_threads, cores=cores, reset_on_connect=not warm, keep_state=warm,
                                              class_ports=getattr(args, "class_ports", None), pair_ports=getattr(args, "pair_ports", None)))
        if n > 1:
            door = ingest.FrontDoor(shards, args.port_num_in, args.port_num_out, bind_any=args.bind_any)
    except Exception:
        teardown(engines, shards, door)
        raise
    return engines, shards, door, mode


def run_worker(args) -> int:
    """One GPU's worker process behind a front-door process: engine + passive front-end, connections arrive over the link (``--worker-link``)."""
    import os
    from . import dist_util, engine, ingest
    stop = {"now": False}
    signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("now", True))
    signal.signal(signal.SIGINT, signal.SIG_IGN)               # ^C goes to the whole foreground group: the door process stops us in order
    r = args.worker_rank
    try:
        blob, mode = load_blob(args)
        dev = 0 if args.share_gpu else r
        eng = engine.Engine(blob, args.vap_process_rate, args.context_len_sec, max_streams=args.streams, max_batch=min(args.streams, args.max_batch),
                            mode=mode, device_id=dev, groups=2, split_f16=(args.precision == "split"), **rate_kw(args))
        warm = load_state(state_path(args.load_state, r, max(1, args.gpus), worker=True), eng, f"GPU {r}: ")
        cores = None
        if args.pin:
            nthr = 1 + args.rx_threads + args.tx_threads
            cores, _ = dist_util.front_end_placement(dev, nthr, skip=(r * nthr if args.share_gpu else 0))
        shard = ingest.NativeServer(eng, port_in=-1, port_out=-1, gain=args.audio_gain, max_wait_s=args.max_wait_ms * 1e-3,
                                    rx_threads=args.rx_threads, tx_threads=args.tx_threads, cores=cores, reset_on_connect=not warm, keep_state=warm)
        shard.attach_link(args.worker_link)
    except Exception as e:                                      # noqa: BLE001
        print(f"[vapx] GPU {r}: worker start-up failed: {e}", file=sys.stderr, flush=True)
        return 1
    parent = os.getppid()
    last = time.time()
    while not stop["now"] and os.getppid() == parent:          # an orphaned worker (the door process died) stops too
        time.sleep(0.2)
        if args.stats_sec > 0 and time.time() - last >= args.stats_sec:
            last = time.time()
            st = shard.stats(reset_latency_window=True)
            print(f"[vapx] GPU {r}: " + json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}), flush=True)
    shard.close()
    save_state(state_path(args.save_state, r, max(1, args.gpus), worker=True), eng, f"GPU {r}: ")
    eng.close()
    return 0


def run_door(args, argv) -> int:
    """The front-door process of ``--worker-procs``: spawns one worker per GPU, owns the port pair, touches no GPU."""
    import subprocess
    from . import ingest
    stop = {"now": False}
    signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("now", True))
    signal.signal(signal.SIGINT, lambda *_: stop.__setitem__("now", True))
    n = max(1, args.gpus)
    mode = args.mode
    if args.precision == "auto":                                # plan once, here; the workers are told the result
        if mode is None and args.synthetic_weights is None:
            from . import checkpoints
            mode = checkpoints.infer_mode(checkpoints.load_state_dicts(args.vap_model, args.cpc_model)[1])
        try:
            choose_precision(args, mode or "vap")
        except Exception as e:                                  # noqa: BLE001
            print(f"[vapx] start-up failed: {e}", file=sys.stderr, flush=True)
            return 1
    base = [a for a in (argv if argv is not None else sys.argv[1:])]
    for flag in ("--precision", "--worker-procs"):              # the workers get the decided values
        while flag in base:
            k = base.index(flag)
            del base[k:k + 2]
    links, workers = [], []
    door = None
    try:
        for r in range(n):
            mine, theirs = ingest.link_pair()
            workers.append(subprocess.Popen([sys.executable, "-u", "-m", "vap_realtime_amd.serve"] + base + ["--precision", args.precision, "--worker-link",
                                             str(theirs.fileno()), "--worker-rank", str(r)], pass_fds=[theirs.fileno()]))
            theirs.close()
            links.append(mine)
        door = ingest.RemoteFrontDoor(links, args.port_num_in, args.port_num_out, bind_any=args.bind_any)
    except Exception as e:                                      # noqa: BLE001
        print(f"[vapx] start-up failed: {e}", file=sys.stderr, flush=True)
        for w in workers:
            w.terminate()
        return 1
    print(f"[vapx] {n} GPU(s) x {args.streams} dialogue slots in {n} worker processes, mode {mode or ('vap' if args.synthetic_weights is not None else 'from the state dict')}, {args.precision} arithmetic, "
          f"{args.vap_process_rate} Hz / {args.context_len_sec} s, audio at {args.input_rate} Hz ({args.input_format}) — input :{door.port_in}, output :{door.port_out} (front-door process: dialogue k -> GPU k mod N)", flush=True)
    rc = 0
    while not stop["now"]:
        time.sleep(0.2)
        dead = [r for r, w in enumerate(workers) if w.poll() is not None]
        if len(dead) == n:                                       # nobody left to serve
            print("[vapx] every worker has exited", file=sys.stderr, flush=True)
            rc = 1
            break
    door.close()
    for w in workers:
        if w.poll() is None:
            w.terminate()
    for w in workers:
        try:
            w.wait(timeout=300 if args.save_state else 30)         # a worker writes its snapshot before it exits
        except Exception:                                        # noqa: BLE001
            w.kill()
    for l in links:
        l.close()
    return rc


def teardown(engines, shards, door, save_path=None):
    if door is not None:
        door.close(close_shards=False)
    for s in shards:
        s.close()
    for r, e in enumerate(engines):
        if save_path:                                            # every front-end is closed: nobody else steps the engines now
            save_state(state_path(save_path, r, len(engines)), e, f"GPU {r}: ")
        e.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vap_model", type=str, default="../../asset/vap/vap_state_dict_jp_20hz_2500msec.pt")
    ap.add_argument("--cpc_model", type=str, default="../../asset/cpc/60k_epoch4-d0f474de.pt")
    ap.add_argument("--port_num_in", type=int, default=50007)
    ap.add_argument("--port_num_out", type=str, default=None, help="50008; with --mode a+b[+c] one port per model, comma-separated (default 50008, 50009, ...)")
    ap.add_argument("--vap_process_rate", type=str, default="20", help="20; with --mode a+b[+c] optionally one rate per model, comma-separated")
    ap.add_argument("--context_len_sec", type=str, default="2.5", help="2.5; with --mode a+b[+c] optionally one window per model, comma-separated")
    ap.add_argument("--gpu", action="store_true", help="accepted for compatibility: this engine has no CPU path")
    ap.add_argument("--audio_gain", type=float, default=1.0)
    ap.add_argument("--mode", type=str, default=None,
                    help="head set: vap, bc or nod (default: inferred from the state dict), or a+b[+c] of distinct ones: several models on one shared "
                         "CPC trunk, the first leads (then --vap_model takes one path per model, comma-separated)")
    ap.add_argument("--input_rate", type=int, choices=[8000, 16000, 32000, 48000], default=16000,
                    help="sample rate of the clients' audio: every packet still carries 10 ms (input_rate / 100 sample pairs); other rates than "
                         "16000 are resampled on the GPU with torchaudio's default filter, which delays the audio by 0.44 - 0.88 ms; the rate "
                         "travels in --save_state / --load_state files")
    ap.add_argument("--input_format", choices=["f64", "s16", "mulaw", "alaw"], default="f64",
                    help="sample format of the clients' audio on the input port: f64 (default) is the reference's framing, 160 x {f64, f64} per "
                         "10 ms; s16 (16-bit little-endian PCM) and mulaw / alaw (G.711) packets carry input_rate / 100 interleaved (ch1, ch2) pairs "
                         "of 2 or 1 bytes per sample and are decoded on the GPU; result packets are unchanged.  Not with --audio_gain")
    ap.add_argument("--input_class", action="append", default=None, metavar="FORMAT@RATE[+FORMAT@RATE][:PORT]",
                    help="repeatable: one INPUT PORT per kind of client on ONE engine, e.g. --input_class f64@16000:50007 --input_class mulaw@8000:50017 "
                         "--input_class s16@48000:50027 (formats and rates as --input_format / --input_rate; PORT 0 or left out = ephemeral); "
                         "A+B, e.g. s16@48000+mulaw@8000:50037, is a PAIR port for dialogues whose channel 1 arrives as A and channel 2 as B, in planar "
                         "10 ms packets (channel 1's 10 ms, then channel 2's); the engine's classes are the distinct ones named anywhere; "
                         "--port_num_in is then ignored.  Not with --input_rate / --input_format, --mode a+b, --gpus N > 1, --save_state / --load_state")
    ap.add_argument("--streams", type=int, default=1, help="dialogue slots per GPU (the reference serves exactly one)")
    ap.add_argument("--max_batch", type=int, default=1024)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--allow-overload", dest="allow_overload", action="store_true",
                    help="with --precision auto: start even when no arithmetic path holds <= 10 ms per frame at --streams dialogues per GPU")
    ap.add_argument("--precision", choices=["auto", "fp32", "split"], default="auto",
                    help="auto (default): fp32 while --streams x rate keeps the fp32 path <= 85 %% busy, else split, refusing loads neither path holds "
                         "within 10 ms (capacity.plan; the choice is printed).  fp32: every contraction on the fp32 MFMA (safe next to other tenants).  split: VAPX_FLAG_SPLIT_F16 — the same "
                         "contractions as fp32-accurate 3-term f16 split products, ~2x the streams per GPU at the same <= 1e-4 parity; for a "
                         "DEDICATED GPU/node (a process that issues f16 MFMAs all day can disturb co-running tenants: DESIGN.md \"co-running f16 MFMA\")")
    ap.add_argument("--share-gpu", dest="share_gpu", action="store_true", help="plumbing check on a 1-GPU box: every shard's engine on device 0")
    ap.add_argument("--max_wait_ms", type=float, default=2.0)
    ap.add_argument("--rx_threads", type=int, default=4)
    ap.add_argument("--tx_threads", type=int, default=4)
    ap.add_argument("--bind_any", action="store_true", help="listen on 0.0.0.0 instead of 127.0.0.1")
    ap.add_argument("--pin", dest="pin", action="store_true",
                    help="pin every shard's tick / receive / sender threads to consecutive cores at the top of its GPU's NUMA node (default: the "
                         "scheduler places them).  Worth it on a host you own — keep everything else off those cores; on a shared host it measured "
                         "no better than floating threads (profiles/r05_frontend/README.md)")
    ap.add_argument("--stats_sec", type=float, default=10.0)
    ap.add_argument("--synthetic-weights", dest="synthetic_weights", type=int, default=None)
    ap.add_argument("--load_state", type=str, default=None,
                    help="snapshot to import before the front-end opens (PATH.<rank> per engine with --gpus N / worker processes); a missing file is a "
                         "warning and a cold start, a file that does not fit the engines is refused")
    ap.add_argument("--save_state", type=str, default=None,
                    help="snapshot of every dialogue slot, written after the front-end has closed on SIGTERM / SIGINT (same naming)")
    ap.add_argument("--worker-procs", dest="worker_procs", choices=["auto", "on", "off"], default="auto",
                    help="one worker PROCESS per GPU behind a front-door process that passes accepted connections on (auto: when one process could not "
                         "hold 2 sockets per dialogue under RLIMIT_NOFILE; --gpus 8 x --streams 4096 needs 65 792 descriptors)")
    ap.add_argument("--worker-link", dest="worker_link", type=int, default=None, help=argparse.SUPPRESS)     # set by the door process
    ap.add_argument("--worker-rank", dest="worker_rank", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    args.port_num_out_default = args.port_num_out is None
    if args.port_num_out is None:
        args.port_num_out = "50008"
    try:
        names = group_modes(args.mode)
        if names is None:
            args.port_num_out = int(args.port_num_out)
            args.vap_process_rate = per_model(args.vap_process_rate, 1, int, "--vap_process_rate")[0]
            args.context_len_sec = per_model(args.context_len_sec, 1, float, "--context_len_sec")[0]
        else:
            args.group_plan = group_plan(args, names)
        args.input_classes = args.class_ports = args.pair_ports = None
        if args.input_class:
            from . import ingest
            args.input_classes, args.class_ports, args.pair_ports = ingest.input_ports(args.input_class)
    except ValueError as e:
        ap.error(str(e))
    why = input_class_refusal(args, names)
    if why:
        ap.error(why)
    if names is not None:
        if args.gpus > 1 or args.worker_procs == "on" or args.worker_link is not None:
            print(f"[vapx] --mode {args.mode} serves one GPU from one process: the front door (--gpus > 1, --worker-procs on) is single-model",
                  file=sys.stderr, flush=True)
            return 2
        stop = {"now": False}
        signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("now", True))
        signal.signal(signal.SIGINT, lambda *_: stop.__setitem__("now", True))
        return run_group(args, names, stop)
    if args.worker_link is not None:
        return run_worker(args)
    if wants_worker_procs(args):
        return run_door(args, argv)
    stop = {"now": False}
    signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("now", True))   # the normal service-stop signal: shut every GPU down in order
    signal.signal(signal.SIGINT, lambda *_: stop.__setitem__("now", True))
    try:
        engines, shards, door, mode = build(args)
    except Exception as e:                                      # noqa: BLE001
        print(f"[vapx] start-up failed: {e}", file=sys.stderr, flush=True)
        return 1
    pin, pout = (door.port_in, door.port_out) if door else (shards[0].port_in, shards[0].port_out)
    if args.input_classes:
        name = lambda c: f"{'f64' if args.input_classes[c][0] == 'f32' else args.input_classes[c][0]}@{args.input_classes[c][1]}"      # noqa: E731
        audio = "input classes " + ", ".join([f"{name(c)} :{port}" for c, port in enumerate(shards[0].class_ports)] +
                                             [f"{name(c1)}+{name(c2)} :{port}" for (c1, c2, _), port in zip(args.pair_ports, shards[0].pair_ports)])
        print(f"[vapx] 1 GPU(s) x {args.streams} dialogue slots, mode {mode}, {args.precision} arithmetic, {args.vap_process_rate} Hz / {args.context_len_sec} s, "
              f"{audio} — output :{pout}", flush=True)
    else:
        print(f"[vapx] {len(engines)} GPU(s) x {args.streams} dialogue slots, mode {mode}, {args.precision} arithmetic, {args.vap_process_rate} Hz / {args.context_len_sec} s, audio at {args.input_rate} Hz ({args.input_format}) — "
          f"input :{pin}, output :{pout}" + (" (front door: dialogue k -> GPU k mod N)" if door else ""), flush=True)
    last = time.time()
    while not stop["now"]:
        time.sleep(0.2)
        if args.stats_sec > 0 and time.time() - last >= args.stats_sec:
            last = time.time()
            for r, s in enumerate(shards):
                st = s.stats(reset_latency_window=True)
                print(f"[vapx] GPU {r}: " + json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}), flush=True)
    teardown(engines, shards, door, args.save_state)
    return 0


if __name__ == "__main__":
    sys.exit(main())
