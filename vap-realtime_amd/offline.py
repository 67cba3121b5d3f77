"""Offline batch driver: many stereo recordings through one engine, output
identical in format to the reference's ``rvap/vap_main/vap_offline.py`` (``time_sec,p_now(0=left),
p_now(1=right),p_future(0=left),p_future(1=right)``, one row per VAP frame) so that
``output/offline_prediction_visualizer`` keeps working.

Framing follows ``vap_offline.py:47-61``: a window of ``frame = 16000//rate + 320`` samples slides by
``frame - 320``; the first window starts at sample 0 (its 320 "carry" samples are real audio, not zeros);
``time = (i + frame) / 16000``.  Here ALL dialogues advance in lock-step, one ``vapx_step`` per frame
index, dialogues that have run out of audio simply drop out of the batch (ragged stream ids).

Recordings at 8, 32 or 48 kHz (``--resample``): an engine with that input rate resamples on the device (``resample.py``).  Its input is
framed in hops of ``rate // frame_rate`` samples from a ZERO carry, as the TCP server frames a connection — a full frame with real carry
samples is defined at 16 kHz only.  The ``time_sec`` rows of such a pair therefore follow the server's framing, ``(f + 1) * hop / 16000``
for frame ``f``, not ``vap_offline.py``'s first-window rule, and the model sees the audio 0.44 - 0.88 ms late (the filter's delay).
"""
from __future__ import annotations

import wave
from typing import Dict, List, Sequence, Tuple

import numpy as np

SR = 16000
RESAMPLED_RATES = (8000, 32000, 48000)
HEADER = "time_sec,p_now(0=left),p_now(1=right),p_future(0=left),p_future(1=right)\n"


def read_wav_mono(path: str):
    """16-bit / 32-bit PCM or float wav -> float32 in [-1, 1] (what ``sf.read(dtype='float32')`` yields).  A 16 kHz file gives the
    samples; a file at 8, 32 or 48 kHz gives ``(samples, rate)`` for an engine with that input rate; any other rate raises."""
    with wave.open(path, "rb") as w:
        rate = w.getframerate()
        if rate != SR and rate not in RESAMPLED_RATES:
            raise ValueError(f"{path}: expected {SR} Hz, got {rate}")
        n, ch, sw = w.getnframes(), w.getnchannels(), w.getsampwidth()
        raw = w.readframes(n)
    if sw == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif sw == 4:
        x = np.frombuffer(raw, "<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported sample width {sw}")
    x = x.reshape(-1, ch)[:, 0].copy()
    return x if rate == SR else (x, rate)


def frame_starts(n_samples: int, frame: int) -> range:
    """Start offsets of the windows ``vap_offline.py:51-54`` processes."""
    shift = frame - 320
    last = n_samples - frame
    return range(0, last + 1, shift) if last >= 0 else range(0)


def run_offline(vap, dialogues: Sequence[Tuple[np.ndarray, np.ndarray]], on_numeric: str = "raise") -> List[List[Dict]]:
    """``vap``: object with ``.hop`` and ``.process(frames[n,2,hop+320], stream_ids) -> dict`` (``ManyStreamVAP``).
    ``dialogues``: (left, right) float32 arrays.  Returns per dialogue the list of
    ``{"t", "p_now", "p_future"}`` rows.

    ``on_numeric``: a recording with a NaN / Inf sample poisons its LSTM state for good.  The reference keeps going and writes
    ``nan`` rows for the rest of that file (``vap_offline.py:62-73`` has no check); the default here is to FAIL (``"raise"``: a batch
    job should not fill files with ``nan`` silently).  ``"reference"`` reproduces the reference: the poisoned dialogue's rows are
    ``nan`` from that frame on, every other dialogue of the batch is unaffected (streams are independent)."""
    if on_numeric not in ("raise", "reference"):
        raise ValueError("on_numeric must be 'raise' or 'reference'")
    frame = vap.hop + 320
    starts = [frame_starts(min(len(l), len(r)), frame) for l, r in dialogues]
    n_frames = [len(s) for s in starts]
    results: List[List[Dict]] = [[] for _ in dialogues]
    for f in range(max(n_frames, default=0)):
        ids = [d for d in range(len(dialogues)) if f < n_frames[d]]
        batch = np.empty((len(ids), 2, frame), np.float32)
        for k, d in enumerate(ids):
            i = starts[d][f]
            batch[k, 0] = dialogues[d][0][i:i + frame]
            batch[k, 1] = dialogues[d][1][i:i + frame]
        out = (vap.process(batch, np.asarray(ids, np.int32)) if on_numeric == "raise"
               else vap.process(batch, np.asarray(ids, np.int32), on_numeric="status"))
        for k, d in enumerate(ids):
            results[d].append({"t": float(starts[d][f] + frame) / SR,
                               "p_now": [float(v) for v in out["p_now"][k]],
                               "p_future": [float(v) for v in out["p_future"][k]]})
    return results


def run_offline_hops(vap, dialogues: Sequence[Tuple[np.ndarray, np.ndarray]], on_numeric: str = "raise") -> List[List[Dict]]:
    """The same for an engine with an input rate: ``vap`` has ``.hop`` (16 kHz) and ``.hop_in`` and takes ``[n,2,hop_in]``.  Every dialogue
    is cut into hops from sample 0 and starts from a zero carry, like a connection to the server; ``t`` of frame ``f`` is the time of
    its last sample, ``(f + 1) * hop / 16000``."""
    if on_numeric not in ("raise", "reference"):
        raise ValueError("on_numeric must be 'raise' or 'reference'")
    hop_in = vap.hop_in
    n_frames = [min(len(l), len(r)) // hop_in for l, r in dialogues]
    results: List[List[Dict]] = [[] for _ in dialogues]
    for f in range(max(n_frames, default=0)):
        ids = [d for d in range(len(dialogues)) if f < n_frames[d]]
        batch = np.empty((len(ids), 2, hop_in), np.float32)
        for k, d in enumerate(ids):
            batch[k, 0] = dialogues[d][0][f * hop_in:(f + 1) * hop_in]
            batch[k, 1] = dialogues[d][1][f * hop_in:(f + 1) * hop_in]
        out = (vap.process(batch, np.asarray(ids, np.int32)) if on_numeric == "raise"
               else vap.process(batch, np.asarray(ids, np.int32), on_numeric="status"))
        for k, d in enumerate(ids):
            results[d].append({"t": float((f + 1) * vap.hop) / SR,
                               "p_now": [float(v) for v in out["p_now"][k]],
                               "p_future": [float(v) for v in out["p_future"][k]]})
    return results


def write_csv(path: str, rows: List[Dict]) -> None:
    """Same text as ``vap_offline.py:76-86`` (``str()`` of Python floats)."""
    with open(path, "w") as f:
        f.write(HEADER)
        for r in rows:
            f.write(str(r["t"]) + "," + str(r["p_now"][0]) + "," + str(r["p_now"][1]) + ","
                    + str(r["p_future"][0]) + "," + str(r["p_future"][1]) + "\n")


def main(argv=None):
    import argparse
    import torch
    from . import realtime
    ap = argparse.ArgumentParser(description="Many-dialogue offline VAP (reference: rvap/vap_main/vap_offline.py)")
    ap.add_argument("--vap_model", required=True)
    ap.add_argument("--cpc_model", required=True)
    ap.add_argument("--pairs", nargs="+", required=True, help="left.wav:right.wav[:out.txt] ...")
    ap.add_argument("--vap_process_rate", type=int, default=20)
    ap.add_argument("--context_len_sec", type=float, default=5)
    ap.add_argument("--on_numeric", choices=["raise", "reference"], default="raise",
                    help="a NaN / Inf sample: fail (default) or, like the reference, keep writing nan rows for that file")
    ap.add_argument("--resample", action="store_true",
                    help="accept pairs at 8, 32 or 48 kHz: they run through an engine with that input rate, framed in hops from a zero carry "
                         "like the server (time_sec then follows the server's framing); default: refuse anything but 16 kHz")
    args = ap.parse_args(argv)
    cpc_sd, vap_sd = realtime._load_state_dicts(args.vap_model, args.cpc_model)
    specs = [p.split(":") for p in args.pairs]
    by_rate: Dict[int, List[int]] = {}
    dialogues = []
    for k, s in enumerate(specs):
        pair = []
        for path in s[:2]:
            got = read_wav_mono(path)
            x, rate = got if isinstance(got, tuple) else (got, SR)
            if rate != SR and not args.resample:
                raise ValueError(f"{path}: expected {SR} Hz, got {rate} (--resample runs 8, 32 and 48 kHz pairs through the engine's resampler)")
            pair.append((x, rate))
        if pair[0][1] != pair[1][1]:
            raise ValueError(f"{s[0]} and {s[1]}: the two channels of a dialogue must have one sample rate")
        dialogues.append((pair[0][0], pair[1][0]))
        by_rate.setdefault(pair[0][1], []).append(k)
    for rate, ks in sorted(by_rate.items()):               # one engine per sample rate
        vap = realtime.ManyStreamVAP(cpc_sd, vap_sd, args.vap_process_rate, args.context_len_sec, n_streams=len(ks), input_hz=rate)
        run = run_offline if rate == SR else run_offline_hops
        for k, rows in zip(ks, run(vap, [dialogues[k] for k in ks], on_numeric=args.on_numeric)):
            out = specs[k][2] if len(specs[k]) > 2 else f"output_offline_{k}.txt"
            write_csv(out, rows)
            print("Generated output file: ", out)
        vap.engine.close()


if __name__ == "__main__":
    main()
