"""Times the two launches of `consistencytta_amd.data.read_wav_batch` (ctta_resample_sinc + ctta_wave_prepare) on the batch
of one fused optimizer step: 45 clips of 10 s at 44100 -> 16000 (segment 163840 samples, the training loader) and at
16000 -> 48000 (segment 480000, the CLAP path).  File reading and the upload are not timed: the clips are random PCM16 / 32768
already on the device.  Prints one JSON line per shape: device-event times per call (median and minimum over --iters calls
after --warmup), the taps the definition needs (counted from the shapes: every output has (n_win - offset) // index_step taps
per wing away from the edges) and, with --step-ms, the launches' share of that optimizer step.

--step-ms is `ms_per_optimizer_step` of the `grad_accum_5_fused_pipelined` leg of `bench.py --gpus 1` measured on the same
machine (--bench-json reads it from a file holding bench.py's result line).  Kernel times proper come from a separate run
under `rocprofv3 --kernel-trace --stats -- python tools/resample_bench.py`.  Nothing here is a comparison with resampy on the
CPU: the package is not installed where this was built and its cost was never measured."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consistencytta_amd import audio, data  # noqa: E402


def step_ms_from(path):
    """`ms_per_optimizer_step` of the grad_accum_5_fused_pipelined leg, wherever bench.py's result line nests it."""
    def find(node):
        if isinstance(node, dict):
            leg = node.get("grad_accum_5_fused_pipelined")
            if isinstance(leg, dict) and "ms_per_optimizer_step" in leg:
                return float(leg["ms_per_optimizer_step"])
            for v in node.values():
                got = find(v)
                if got is not None:
                    return got
        return None

    for line in open(path):
        if line.startswith('{"metric"'):
            got = find(json.loads(line))
            if got is not None:
                return got
    sys.stderr.write("%s holds no grad_accum_5_fused_pipelined leg with ms_per_optimizer_step: no share printed\n" % path)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=45)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=None)
    ap.add_argument("--bench-json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    step_ms = a.step_ms if a.step_ms is not None else (step_ms_from(a.bench_json) if a.bench_json else None)
    dev = torch.device("cuda", torch.cuda.current_device())
    win, num_table = audio.resampy_filter("kaiser_best")
    n_win = win.shape[0]
    for sr_orig, sr_new, segment in ((44100, 16000, 163840), (16000, 48000, 480000)):
        B, n_in = a.clips, int(a.seconds * sr_orig)
        g = torch.Generator().manual_seed(sr_orig)
        x = (torch.randint(-32768, 32768, (B, n_in), generator=g).float() / 32768.0).to(dev)
        descs, y_off = [], 0
        for b in range(B):
            descs.append(audio.resample_clip(n_in, sr_orig, sr_new, num_table, b * n_in, y_off))
            y_off += descs[-1].n_out
        n_out = descs[0].n_out
        table = audio.clip_table(descs, dev)
        y = torch.empty(y_off, dtype=torch.float32, device=dev)
        lens = [n_out] * B

        def call(events=None):
            if events:
                events[0].record()
            audio.resample_launch(x, y, table, B, n_out)
            if events:
                events[1].record()
            out = data.wave_prepare(y, None, lens, segment, clips=table)
            if events:
                events[2].record()
            return out

        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        t_rs, t_wp = [], []
        for _ in range(a.iters):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            call(ev)
            ev[2].synchronize()
            t_rs.append(ev[0].elapsed_time(ev[1]) * 1e3)
            t_wp.append(ev[1].elapsed_time(ev[2]) * 1e3)
        both = sorted(r + w for r, w in zip(t_rs, t_wp))
        t_rs.sort()
        t_wp.sort()
        taps = B * n_out * 2 * (n_win // descs[0].index_step)
        res = {"clips": B, "sr_orig": sr_orig, "sr_new": sr_new, "n_in": n_in, "n_out": n_out, "segment": segment,
               "resample_us_median": round(t_rs[len(t_rs) // 2], 1), "resample_us_min": round(t_rs[0], 1),
               "prepare_us_median": round(t_wp[len(t_wp) // 2], 1), "prepare_us_min": round(t_wp[0], 1),
               "both_us_median": round(both[len(both) // 2], 1), "gtaps": round(taps / 1e9, 3),
               "gtaps_per_s": round(taps / 1e9 / (t_rs[len(t_rs) // 2] * 1e-6), 1),
               "mbytes_prepare": round(4 * (3 * B * n_out + B * segment) / 1e6, 1)}
        if step_ms:
            res["optimizer_step_ms"] = step_ms
            res["share_of_step"] = round(both[len(both) // 2] * 1e-3 / step_ms, 5)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
