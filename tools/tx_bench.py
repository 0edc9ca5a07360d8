#!/usr/bin/env python3
"""pktout checksum insertion kernel vs the receive validation kernel, timed
interleaved in one process on config 3's IMIX batch (IPv4, 80 % UDP / 20 %
TCP), rotating over 4 device copies:

  (a) mi_cls_chksum_insert, all four pktout defaults on;
  (b) the pktin-option receive kernel (IPv4 / UDP / TCP / SCTP validation)
      under a default-CoS-only program, on the same bytes.

Per launch: time (median and min over the rounds), algorithmic bytes (frame
bytes + 14 B of descriptors per packet for (a), + 22 B of descriptor and
record for (b)) and their fraction of 8 TB/s.  --loop also measures the
loop pktio's send rate (tests/_bin/tx_driver) with and without insertion.

--hash times, interleaved in one process on a 4096-packet batch of the same
traffic, the transmit kernel's three instantiations (checksums alone -- the
kernel of mi_cls_chksum_insert --, checksums with the pktin flow hash, the
hash alone), and --queues N the wall time of an odp_pktout_send call on a
loop pktio with N hashed input queues against one (tests/_bin/mq_driver).

  python tools/tx_bench.py [--n 1000000] [--rounds 7] [--steps 200] [--loop] [--out FILE]
  python tools/tx_bench.py --hash [--queues 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def span_ms(torch, stream, steps, fn, args):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for i in range(steps):
        rc = fn(*args[i % len(args)])
        if rc:
            raise RuntimeError(f"launch failed: {rc}")
    ev1.record(stream)
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps


def kernels(a):
    import torch

    from odp_amd import _build
    from odp_amd import rules as R
    from odp_amd.cls import TX_DESC_DTYPE, Classifier, TxContext
    _build.build()
    b, _ = R.config3(a.n)
    desc = np.zeros(b.n, TX_DESC_DTYPE)
    desc["l3"], desc["l4"] = 14, 34
    if not torch.cuda.is_available():
        raise SystemExit("tx_bench: no GPU")
    dev = torch.device("cuda:0")
    c = Classifier(gpu=0)
    c.apply([R.cos("default", queue=1), ("default", 0)])
    c.set_pktin_opt(0x3C)
    c.spec_wait()
    t = TxContext(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    tx_args, rx_args = [], []
    keep = []
    for _ in range(a.rotate):
        tb = torch.from_numpy(b.buf).to(dev)
        to = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        tl = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        td = torch.from_numpy(desc.view(np.int64).copy()).to(dev)
        tdone = torch.zeros(b.n, dtype=torch.uint8, device=dev)
        tout = torch.empty((b.n, 4), dtype=torch.int32, device=dev)
        keep += [tb, to, tl, td, tdone, tout]
        tx_args.append((tb.data_ptr(), to.data_ptr(), tl.data_ptr(), td.data_ptr(), b.n, 0xF0,
                        tdone.data_ptr(), stream))
        rx_args.append((tb.data_ptr(), to.data_ptr(), tl.data_ptr(), b.n, tout.data_ptr(), stream))
    cur = torch.cuda.current_stream(dev)
    # warm-up of both (the insert first: every timed launch of either kernel
    # then sees the same bytes, checksums in place)
    span_ms(torch, cur, 2 * a.rotate, t.insert_device, tx_args)
    span_ms(torch, cur, 2 * a.rotate, c.classify_device, rx_args)
    tx_ms, rx_ms = [], []
    for _ in range(a.rounds):
        tx_ms.append(span_ms(torch, cur, a.steps, t.insert_device, tx_args))
        rx_ms.append(span_ms(torch, cur, a.steps, c.classify_device, rx_args))
    ll = c.last_launch()
    done = keep[4].cpu().numpy()
    errs = keep[5].cpu().numpy().view(np.uint8).reshape(-1).view(R.RESULT_DTYPE)["err"]
    frame = int(b.len.astype(np.int64).sum())

    def line(ms, per_pkt):
        by = frame + per_pkt * b.n
        med, mn = statistics.median(ms), min(ms)
        return {"us_per_launch_median": round(1e3 * med, 2), "us_per_launch_min": round(1e3 * mn, 2),
                "rounds_us": [round(1e3 * x, 2) for x in ms], "bytes_per_launch": by,
                "frac_of_8TBps_median": round(by / (med * 1e-3) / HBM_PEAK, 4),
                "mpkts_per_s_median": round(b.n / (med * 1e-3) / 1e6, 1)}

    res = {"packets": b.n, "frame_bytes": frame, "rotate": a.rotate, "steps": a.steps,
           "rounds": a.rounds,
           "insert": dict(line(tx_ms, 14), kernel="mi_cls_tx_kernel", pktout_opt="0xF0",
                          inserted_all=bool((done != 0).all())),
           "validate": dict(line(rx_ms, 22), kernel=ll["name"], pktin_opt="0x3C",
                            checksum_errors=int((errs & 0x44 != 0).sum()))}
    res["insert_over_validate_median"] = round(
        res["insert"]["us_per_launch_median"] / res["validate"]["us_per_launch_median"], 3)
    t.close()
    c.close()
    return res


def loop_rate(a):
    """Send rate of the loop pktio (time inside odp_pktout_send), insertion on
    and off, alternating."""
    import tempfile

    from odp_amd import rules as R
    from tests.rt_helpers import write_pcap
    b, _ = R.config3(a.loop_frames)
    frames = [b.frame(i) for i in range(b.n)]
    drv = os.path.join(ROOT, "tests", "_bin", "tx_driver")
    out = {"frames": b.n, "with_insert_mpps": [], "without_mpps": []}
    with tempfile.TemporaryDirectory() as d:
        pcap = os.path.join(d, "imix.pcap")
        write_pcap(pcap, frames)
        env = dict(os.environ, TX_COUNT_ONLY="1", TX_POOL_NUM=str(b.n + 1024))
        for _ in range(3):
            for key, bits in (("with_insert_mpps", "0xF0"), ("without_mpps", "0x0")):
                r = subprocess.run([drv, "loop", pcap, bits, "0x3C", "0"], stdout=subprocess.PIPE,
                                   stderr=subprocess.PIPE, text=True, timeout=120, env=env)
                if r.returncode:
                    raise RuntimeError(f"tx_driver rc={r.returncode}: {r.stderr[-500:]}")
                w = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")][0]
                out[key].append(round(int(w[1]) / int(w[2]) * 1e3, 2))
    return out


def hash_kernels(a):
    """Back-to-back launches between two device events (so a launch's time
    includes what the queue adds between kernels), the three instantiations
    alternating inside every round."""
    import torch

    from odp_amd import _build
    from odp_amd import rules as R
    from odp_amd.cls import TX_DESC_DTYPE, TxContext
    _build.build()
    if not torch.cuda.is_available():
        raise SystemExit("tx_bench: no GPU")
    n = 4096
    b, _ = R.config3(n)
    desc = np.zeros(b.n, TX_DESC_DTYPE)
    desc["l3"], desc["l4"] = 14, 34
    proto = b.buf[b.off.astype(np.int64) + 23]
    desc["flags"] = 0x40 | np.where(proto == 17, 0x10, np.where(proto == 6, 0x20, 0)).astype(np.uint8)
    dev = torch.device("cuda:0")
    t = TxContext(0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ck, both, alone, keep = [], [], [], []
    for _ in range(a.rotate):
        tb = torch.from_numpy(b.buf).to(dev)
        to = torch.from_numpy(b.off.astype(np.uint32).view(np.int32)).to(dev)
        tl = torch.from_numpy(b.len.astype(np.uint16).view(np.int16)).to(dev)
        td = torch.from_numpy(desc.view(np.int64).copy()).to(dev)
        tdone = torch.zeros(b.n, dtype=torch.uint8, device=dev)
        th = torch.zeros(b.n, dtype=torch.int32, device=dev)
        keep += [tb, to, tl, td, tdone, th]
        p = (tb.data_ptr(), to.data_ptr(), tl.data_ptr(), td.data_ptr(), b.n, 0xF0, tdone.data_ptr())
        ck.append(p + (stream,))
        both.append(p + (63, th.data_ptr(), True, stream))
        alone.append(p + (63, th.data_ptr(), False, stream))
    cur = torch.cuda.current_stream(dev)
    variants = (("chksum", t.insert_device, ck), ("chksum_hash", t.hash_device, both),
                ("hash", t.hash_device, alone))
    for _, fn, args in variants:
        span_ms(torch, cur, 50 * a.rotate, fn, args)
    ms = {k: [] for k, _, _ in variants}
    steps = max(a.steps, 2000)
    for _ in range(a.rounds):
        for k, fn, args in variants:
            ms[k].append(span_ms(torch, cur, steps, fn, args))
    from tests import txq_model as TQ
    exp, _ = TQ.apply(b.buf, b.off, b.len, desc, 63)
    same = bool(np.array_equal(keep[5].cpu().numpy().view(np.uint32), exp))
    t.close()
    res = {"packets": b.n, "frame_bytes": int(b.len.astype(np.int64).sum()), "steps": steps, "rounds": a.rounds,
           "hash_equals_model": same}
    for k in ms:
        res[k] = {"us_per_launch_median": round(1e3 * statistics.median(ms[k]), 3),
                  "us_per_launch_min": round(1e3 * min(ms[k]), 3),
                  "rounds_us": [round(1e3 * x, 3) for x in ms[k]]}
    res["chksum_hash_over_chksum_median"] = round(
        res["chksum_hash"]["us_per_launch_median"] / res["chksum"]["us_per_launch_median"], 4)
    return res


def queue_send(a):
    """Wall time of an odp_pktout_send call (256 packets) on a loop pktio:
    one input queue against a.queues hashed ones, with and without pktout
    checksums, alternating."""
    import tempfile

    from odp_amd import rules as R
    from tests.rt_helpers import write_pcap
    b, _ = R.config3(a.loop_frames)
    drv = os.path.join(ROOT, "tests", "_bin", "mq_driver")
    keys = [(f"q{nq}_{'chksum' if bits != '0x0' else 'plain'}", nq, bits)
            for bits in ("0x0", "0xF0") for nq in (1, a.queues)]
    out = {"frames": b.n, "burst": 256, "queues": a.queues, "us_per_send_call": {k: [] for k, _, _ in keys},
           "launches": {}}
    with tempfile.TemporaryDirectory() as d:
        pcap = os.path.join(d, "imix.pcap")
        write_pcap(pcap, [b.frame(i) for i in range(b.n)])
        env = dict(os.environ, TX_COUNT_ONLY="1", TX_POOL_NUM=str(b.n + 1024), MQ_BURST="256")
        for _ in range(3):
            for key, nq, bits in keys:
                r = subprocess.run([drv, "loop", pcap, "direct", str(nq), "0x3f", "1", bits, "0"],
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120,
                                   env=env)
                if r.returncode:
                    raise RuntimeError(f"mq_driver rc={r.returncode}: {r.stderr[-500:]}")
                w = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("R ")][0]
                out["us_per_send_call"][key].append(round(int(w[3]) / int(w[2]) / 1e3, 2))
                out["launches"][key] = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("T ")][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--loop-frames", type=int, default=16384)
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--queues", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.hash:
        res = {"kernels_4096": hash_kernels(a), "send_call": queue_send(a)}
        s = json.dumps(res)
        print(s, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")
        return
    res = kernels(a)

    def emit():
        s = json.dumps(res)
        print(s, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")

    emit()
    if a.loop:
        res["loop_send"] = loop_rate(a)
        emit()


if __name__ == "__main__":
    main()
