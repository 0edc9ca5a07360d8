"""The chain classify -> pool plan -> pool move -> run plan -> vector take / fill
/ enqueue through the public API (tests/rt/vecfill_driver.c), on the runtime's
own packets, page-locked vector pools and queues, against what the existing
receive path delivers for the same capture and control plane (rx_driver): per
queue the events and vector sizes in order, every packet's pool, metadata and
bytes, the pktio counters, the queue stats; and every pool full again at the
end.
"""
import os
import struct
import subprocess
from collections import defaultdict

import pytest

from tests import rt_helpers as H
from tests import zoo

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(H.ROOT, "tests", "_bin", "vecfill_driver")


def run_chain(pcap, rules, frames_path, burst, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([DRIVER, f"pcap:in={pcap}", rules, frames_path, str(burst), "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120, env=e)
    assert r.returncode == 0, f"vecfill_driver rc={r.returncode}\n{r.stderr[-2000:]}"
    queues, events, qstats, free = defaultdict(list), {}, {}, {}
    inside = defaultdict(int)
    stats = counters = None
    for line in r.stdout.splitlines():
        p = line.split()
        if not p:
            continue
        assert p[0] != "SEGMENTED", line
        if p[0] == "V":
            events.setdefault(p[1], []).append(("V", int(p[2])))
            inside[p[1]] = int(p[2])
        elif p[0] == "P":
            if inside[p[1]]:
                inside[p[1]] -= 1
            else:
                events.setdefault(p[1], []).append(("P",))
            q, pool, fl, err, l3, l4, mark, ln, data = p[1:10]
            queues[q].append((pool, int(fl, 16), int(err), int(l3), int(l4), int(mark), int(ln), data))
        elif p[0] == "S":
            stats = tuple(int(x) for x in p[1:5])
        elif p[0] == "Q":
            qstats[(p[1], int(p[2]))] = (int(p[3]), int(p[4]))
        elif p[0] == "F":
            free[p[1]] = (int(p[2]), int(p[3]))
        elif p[0] == "C":
            counters = dict(zip(("vectors", "lost", "holes", "refused", "events"), (int(x) for x in p[1:6])))
    return dict(queues), stats, qstats, events, free, counters


@pytest.mark.parametrize("pktv,burst,short", [("4,100000", 37, False), ("64,100000", 4096, False),
                                              ("8,25", 4096, True)])
def test_chain_equals_the_receive_path(built, gpu, tmp_path, pktv, burst, short):
    """pktv: the vector size and the vector pool's size.  The last case's pool
    runs short: with the whole capture in one burst no vector returns to the
    pool while either path works, so both give the runs their vectors in
    arrival order until it is empty, and the packets left out are queue
    discards in both."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 4)
    assert len(frames) < 4096
    prog = zoo.prog_everything()
    pc, rules, raw = str(tmp_path / "in.pcap"), str(tmp_path / "rules.txt"), str(tmp_path / "frames.bin")
    H.write_pcap(pc, frames)
    H.write_rules(rules, prog)
    with open(raw, "wb") as f:
        f.write(struct.pack("<I", len(frames)))
        for fr in frames:
            f.write(struct.pack("<H", len(fr)) + fr)
    env = {"RX_PKTV": pktv, "ODP_AMD_RX_BURST": str(burst)}
    ev_rx = {}
    # the zoo's program has 47 enqueue CoS and the pool plan tells 16 pools apart: every CoS takes its
    # packets from the pktio's pool (cos_pools 0), in both drivers
    q_rx, s_rx, qs_rx = H.run_driver(f"pcap:in={pc}", rules, "sched", 4, 0, 1, events=ev_rx, env=env)
    q, s, qs, ev, free, ctr = run_chain(pc, rules, raw, burst, env)
    assert ev == ev_rx                                   # per queue: events and vector sizes, in order
    assert sorted(q) == sorted(q_rx)
    for name in q_rx:
        assert q[name] == q_rx[name], name               # pool, flags, error, offsets, mark, length, bytes
    assert s == s_rx
    assert qs == qs_rx                                   # packets and discards per (CoS, queue slot)
    assert free and all(a == b for a, b in free.values()), free
    nvec = sum(e[0] == "V" for v in ev.values() for e in v)
    assert ctr["vectors"] == nvec > 3 and ctr["refused"] == 0 and ctr["holes"] == 0
    assert ctr["events"] == sum(len(v) for v in ev.values())
    discards = sum(d for _, d in qs.values())
    if short:
        assert ctr["lost"] == discards > 0 and nvec == 25
    else:
        assert ctr["lost"] == discards == 0
