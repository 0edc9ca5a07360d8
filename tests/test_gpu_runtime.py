"""End-to-end receive path on the GPU through the ODP runtime subset: frames
enter a pcap or loop pktio, are parsed + classified in GPU bursts
(odp_amd_cls_classify_host -> mi_cls_kernel) and land in CoS queues; the
packets every queue delivers (order, pool, input flags, error bit, l3/l4
offsets, cls mark, bytes) and the pktio / queue counters must be exactly what
the reference receive path produces, derived from the CPU oracle
(tests/rt_helpers.expected).  Also runs the reference's example/classifier,
compiled unchanged against this build, with its own CI arguments
(example/classifier/odp_classifier_run.sh,
platform/linux-generic/test/example/classifier/pktio_env:21-23).
"""
import os
import subprocess

import numpy as np
import pytest

from odp_amd import pktgen as pg
from odp_amd import rules as R
from tests import rt_helpers as H
from tests import zoo

pytestmark = pytest.mark.gpu

UDP64 = os.path.join(H.ROOT, "tests", "golden", "udp64.pcap")


def _run_case(tmp_path, prog, frames, mode="sched", pktio="pcap", cos_pools=1, layer=4, cls=1,
              burst=None, pktin_opt=0, env_extra=None):
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    env = {"ODP_AMD_RX_BURST": str(burst)} if burst else {}
    env.update(env_extra or {})
    if pktin_opt:
        env["RX_PKTIN_OPT"] = str(pktin_opt)
    if pktio == "loop":
        got = H.run_driver("loop", rules, mode, layer, cos_pools, cls, src=pc, env=env)
    else:
        got = H.run_driver(f"pcap:in={pc}", rules, mode, layer, cos_pools, cls, env=env)
    exp = H.expected(prog, frames, cos_pools, cls, layer, pktin_opt=pktin_opt)
    H.compare(got, exp)
    return got


def test_example_classifier_udp64(built, gpu):
    """The reference's own acceptance run: 100 packets to queue1, 100 to
    DefaultCos, exit status 0."""
    # the binary is built in the build container and travels with the tree:
    # missing on the GPU box is a failure, not a skip
    assert os.path.exists(H.EXAMPLE), f"{H.EXAMPLE} missing: run __graft_entry__.build()"
    r = subprocess.run([H.EXAMPLE, "-t", "1", "-i", f"pcap:in={UDP64}", "-m", "0", "-p",
                        "ODP_PMR_SIP_ADDR:10.10.10.0:0xFFFFFF00:queue1", "-P", "-C",
                        "queue1:100", "-C", "DefaultCos:100"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=90,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-3000:]
    # the statistics row: "<queue> <pool>|" per policy, then total
    rows = [ln for ln in r.stdout.splitlines() if ln.count("|") >= 2 and ln[:1].isdigit()]
    assert rows, r.stdout[-3000:]
    cells = [c.split() for c in rows[-1].split("|")[:2]]
    assert [int(x) for x in cells[0]] == [100, 100]   # queue1: queue, pool
    assert [int(x) for x in cells[1]] == [100, 100]   # DefaultCos
    assert "Exit" in r.stdout


def test_example_classifier_two_workers_dmac(built, gpu):
    """Two worker threads, a DMAC rule, no dedicated CoS pools (-d 0)."""
    # the binary is built in the build container and travels with the tree:
    # missing on the GPU box is a failure, not a skip
    assert os.path.exists(H.EXAMPLE), f"{H.EXAMPLE} missing: run __graft_entry__.build()"
    r = subprocess.run([H.EXAMPLE, "-t", "1", "-c", "2", "-d", "0", "-i", f"pcap:in={UDP64}",
                        "-m", "0", "-p", "ODP_PMR_DMAC:02-00-00-00-00-02:ffffffffffff:mac",
                        "-P", "-C", "mac:200"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=90,
                       cwd="/tmp")
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize("mode", ["sched", "direct", "queue"])
def test_rx_zoo_everything(built, gpu, tmp_path, mode):
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_everything(), frames, mode)


def test_rx_zoo_shared_pool(built, gpu, tmp_path):
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_everything(), frames, cos_pools=0)


def test_rx_loop_pktio(built, gpu, tmp_path):
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_everything(), frames, pktio="loop")


# the delivery paths of a burst: the receive chain (default), the GPU delivery
# kernel without it, the host's, and the host's because no pool is page-locked
DELIVERY_ENV = {"gpu": {}, "gpu_no_chain": {"ODP_AMD_RX_CHAIN": "0"},
                "host": {"ODP_AMD_RX_GPU_DELIVER": "0"},
                "pageable_pools": {"ODP_AMD_PINNED_POOLS": "0"}}


@pytest.mark.parametrize("cos_pools", [0, 1])
@pytest.mark.parametrize("delivery", list(DELIVERY_ENV))
def test_rx_delivery_paths(built, gpu, tmp_path, cos_pools, delivery):
    """The receive delivery after classification on every path: the receive
    chain, the GPU delivery kernel without it (ODP_AMD_RX_CHAIN=0; page-locked
    pools: metadata, frame copies and the group-by-queue done by
    mi_cls_deliver_submit; loop packets classified in place, copied only on a
    pool switch) and the host's (ODP_AMD_RX_GPU_DELIVER=0, or pools in
    ordinary memory).  pcap and loop pktios, shared pool (in place) and
    per-CoS pools (pool switch); every queue's packets, metadata and counters
    as the reference's."""
    env = DELIVERY_ENV[delivery]
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    for pktio in ("pcap", "loop"):
        _run_case(tmp_path, zoo.prog_everything(), frames, mode="direct", pktio=pktio,
                  cos_pools=cos_pools, burst=61, env_extra=env)


def test_rx_pktio_pool_held_cos_pools(built, gpu, tmp_path):
    """Every packet of the pktio's pool held by the application while every
    CoS has a pool of its own: the pcap receive keeps moving --
    the frames never need the pktio's pool -- and delivers what the
    reference delivers."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    prog = [op for op in zoo.prog_everything()]
    _run_case(tmp_path, prog, frames, mode="direct", cos_pools=1,
              env_extra={"RX_HOLD_PKTIO_POOL": "1"})


def test_rx_deletes_and_drops(built, gpu, tmp_path):
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_deletes(), frames)
    _run_case(tmp_path, zoo.prog_no_default(), frames)


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_rx_parse_layers_no_classifier(built, gpu, tmp_path, layer):
    """Classifier disabled: packets go to the pktin queue parsed up to the
    configured layer (odp_packet_io.c:675-677, odp_parse.c:372-414)."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, [], frames, cls=0, layer=layer)


def test_rx_random_programs_small_bursts(built, gpu, tmp_path):
    """Random CoS graphs + fuzzed frames, with 37-packet GPU bursts so that
    enqueue runs straddle burst boundaries."""
    rng = np.random.default_rng(1234)
    base = [f for _, f in zoo.all_frames()]
    for it in range(3):
        frames = H.pcap_frames(base + zoo.mutate_frames(rng, base, 300))
        prog = zoo.random_program(rng, base)
        if any(op[0] == "cos" and " " in op[1] for op in prog):
            continue
        _run_case(tmp_path, prog, frames, burst=37)


@pytest.mark.parametrize("layer,opt,cls", [(4, 0x3C, 1), (4, 0x7FC, 1), (4, 0x780, 1),
                                           (2, 0x7FC, 0), (3, 0x7FC, 0), (4, 0x7FC, 0)])
def test_rx_pktin_checksum_options(built, gpu, tmp_path, layer, opt, cls):
    """odp_pktio_config(pktin.bit.*_chksum / drop_*_err) through the runtime:
    checksum statuses (odp_packet_l3/l4_chksum_status), error-CoS routing,
    drops and in_errors as the reference receive path produces them; with the
    classifier off, the parser layer limits which options apply."""
    from tests import chksum_frames as CK
    frames = H.pcap_frames([f for f, _, _ in CK.frame_set(seed=51, n=120)] +
                           [f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_everything(), frames, layer=layer, cls=cls, pktin_opt=opt)


def test_rx_config2_traffic(built, gpu, tmp_path):
    """BASELINE config 2 traffic (16 SIP /24 rules) through the pcap pktio."""
    b, prog = R.config2(20000)
    frames = [b.frame(i) for i in range(b.n)]
    got = _run_case(tmp_path, prog, frames)
    assert sum(len(v) for v in got[0].values()) == 20000


@pytest.mark.parametrize("max_size,burst", [(4, 37), (1, 64), (64, 4096), (7, 1)])
def test_rx_packet_vector_cos(built, gpu, tmp_path, max_size, burst):
    """CoS packet-vector delivery (odp_cls_cos_param_t.vector): the same
    packets, order, metadata and counters as plain delivery, grouped into
    vectors exactly as _odp_cos_vector_enq groups each enqueue run
    (odp_classification_internal.h:83-137)."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 3)
    prog = zoo.prog_everything()
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    ev = {}
    got = H.run_driver(f"pcap:in={pc}", rules, "sched", 4, 1, 1, events=ev,
                       env={"RX_PKTV": f"{max_size},100000", "ODP_AMD_RX_BURST": str(burst)})
    H.compare(got, H.expected(prog, frames, 1, 1, 4))
    exp = H.expected_vectors(prog, frames, burst, max_size)
    assert ev == exp


def test_rx_packet_vector_pool_exhausted(built, gpu, tmp_path):
    """A vector pool too small for the traffic: runs that get no vector are
    dropped and counted as queue discards (odp_classification_internal.h:
    104-108); nothing is lost without a count."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 4)
    prog = zoo.prog_everything()
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    queues, stats, qstats = H.run_driver(f"pcap:in={pc}", rules, "sched", 4, 1, 1,
                                         env={"RX_PKTV": "8,1", "ODP_AMD_RX_BURST": "4096"})
    _, _, eqs = H.expected(prog, frames, 1, 1, 4)
    delivered = sum(len(v) for v in queues.values())
    discards = sum(d for _, d in qstats.values())
    assert delivered + discards == sum(v[0] for v in eqs.values())
    assert discards > 0


def test_rx_hash_queue_event_aggregators(built, gpu, tmp_path):
    """Hash-queue CoS whose queues have event aggregators
    (queue_param.num_aggr): runs go to odp_queue_aggr(q, 0)
    (odp_classification_internal.h:149-157), so every packet of those queues
    arrives inside an event vector; order, metadata and queue stats as plain
    delivery."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 3)
    prog = zoo.prog_everything()
    assert any(op[0] == "cos" and op[2]["num_queue"] > 1 for op in prog)
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    ev = {}
    got = H.run_driver(f"pcap:in={pc}", rules, "sched", 4, 1, 1, events=ev,
                       env={"RX_AGGR": "8", "ODP_AMD_RX_BURST": "41"})
    H.compare(got, H.expected(prog, frames, 1, 1, 4))
    hq = [q for q in got[0] if q.startswith("_odp_cos_hq_")]
    assert hq
    for q in hq:
        assert all(e[0] == "E" and 1 <= e[1] <= 8 for e in ev[q]), ev[q]
        assert sum(e[1] for e in ev[q]) == len(got[0][q])
    for q in got[0]:
        if q not in hq:
            assert all(e == ("P",) for e in ev[q])


def test_rx_small_first_segment(built, gpu, tmp_path):
    """Pools whose pkt.seg_len (64 B) is below the frame sizes: the runtime
    keeps every packet in one segment (seg_len is the minimum first-segment
    length the spec asks for), so the parse sees seg_end = frame_len and the
    reference's segmented-copy path (pktio/loop.c:299-306) has nothing to
    do; rules on bytes deep in 1514-B frames (custom frame offset 1400)
    classify as the oracle says, and every delivered packet is one segment."""
    from odp_amd import pktgen as pg
    frames = [f for _, f in zoo.all_frames()]
    big = [pg.udp4_frame(src=f"10.0.0.{i}", dport=1000 + i, size=1514) for i in range(40)]
    big = [f[:1400] + bytes([i & 0xFF, 0x5A]) + f[1402:] for i, f in enumerate(big)]
    frames = H.pcap_frames(frames + big + frames)
    prog = [R.cos("default", queue=1), R.cos("deep", queue=2), R.cos("v6", queue=3),
            ("default", 0),
            ("pmr", [R.t_custom(R.PMR_CUSTOM_FRAME, 1400, bytes([7, 0x5A]), b"\xff\xff")],
             0, 1, 9),
            ("pmr", [R.t_be16(R.PMR_ETHTYPE_0, pg.ETH_IPV6)], 0, 2, 0)]
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    for pktio in ("pcap", "loop"):
        env = {"RX_SEG_LEN": "64"}
        got = (H.run_driver(f"pcap:in={pc}", rules, "sched", 4, 1, 1, env=env) if pktio == "pcap"
               else H.run_driver("loop", rules, "sched", 4, 1, 1, src=pc, env=env))
        H.compare(got, H.expected(prog, frames, 1, 1, 4))
        assert len(got[0]["deep"]) == 1


@pytest.mark.parametrize("switch_after", [1, 2, 3])
def test_rx_cos_destroyed_while_burst_in_flight(built, gpu, tmp_path, switch_after):
    """A hash-queue CoS is destroyed (its queues with it, and a new default
    CoS with a new queue created) between two odp_pktin_recv calls while
    earlier bursts are still in flight on the GPU: after call 1 the first
    burst is being classified, after calls 2 and 3 the first bursts are in
    their GPU delivery (queues and pools already settled under the old
    tables).  Those bursts must be delivered under the current
    tables (as the synchronous path would), not to the destroyed CoS's queues
    or a queue that reused their slots: every packet the current rules
    enqueue reaches the new CoS, and in_discards counts only the frames the
    oracle discards (compare() checks the pktio counters)."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    before = [R.cos("A", num_queue=4, hash_proto=0x7), ("default", 0)]
    after = [R.cos("B"), ("default", 1), ("cos_destroy", 0)]
    r1, r2 = str(tmp_path / "r1.txt"), str(tmp_path / "r2.txt")
    H.write_rules(r1, before)
    H.write_rules(r2, after)
    # loops=3 (two passes over the capture: the reference's loop count
    # starts at 1, pcap.c:257-278) in bursts of 16: the first call's burst
    # stays in flight (more frames are waiting at the driver)
    got = H.run_driver(f"pcap:in={pc}:loops=3", r1, "direct", 4, 1, 1,
                       env={"ODP_AMD_RX_BURST": "16", "RX_SWITCH_RULES": r2,
                            "RX_SWITCH_AFTER": str(switch_after)})
    exp = H.expected(before + after, frames * 2, 1, 1, 4)
    H.compare(got, exp)
    assert got[0].get("B"), "nothing reached the new default CoS"


def test_rx_mixed_delivery_paths_keep_order(built, gpu, tmp_path):
    """Bursts that alternate between the GPU delivery and the host's (the
    error CoS's pool is in ordinary memory, so a burst holding an error frame
    is delivered on the host at once while older bursts may still be in their
    GPU delivery): every queue still receives its packets in
    arrival order, on pcap and loop pktios, as the reference's synchronous
    receive does (pktio/loop.c:253-384)."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()] * 3)
    for pktio in ("pcap", "loop"):
        _run_case(tmp_path, zoo.prog_everything(), frames, mode="direct", pktio=pktio,
                  cos_pools=1, burst=8, env_extra={"ODP_AMD_PAGEABLE_POOLS": "errPool"})


def test_rx_burst_above_device_grouping(built, gpu, tmp_path):
    """Bursts larger than the delivery kernel's grouping serves
    (MI_CLS_DLV_GROUP_MAX = 8192 entries): the burst is enqueued
    per run instead, nothing is lost and every queue's order and counters are
    the reference's."""
    b, prog = R.config2(20000)
    frames = [b.frame(i) for i in range(b.n)]
    got = _run_case(tmp_path, prog, frames, mode="direct", burst=9000)
    assert sum(len(v) for v in got[0].values()) == 20000


def test_rx_chain_short_pool_redo(built, gpu, tmp_path):
    """The receive chain takes each burst's packets from the CoS pools before
    the GPU decides (as many per pool as the previous bursts needed, plus a
    margin).  Traffic whose CoS mix flips between bursts leaves a pool short:
    that burst is delivered again by the host path, and every queue's packets,
    order, pools and counters stay the reference's."""
    from odp_amd import pktgen as pg
    prog = [R.cos("default", queue=1), R.cos("a", queue=2), R.cos("b", queue=3), ("default", 0),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 1111)], 0, 1, 5),
            ("pmr", [R.t_be16(R.PMR_UDP_DPORT, 2222)], 0, 2, 6)]
    frames = []
    for blk in range(12):
        port = 1111 if blk % 3 == 0 else (2222 if blk % 3 == 1 else 3333)
        frames += [pg.udp4_frame(src=f"10.1.{blk}.{i % 250}", dport=port, size=60 + (i % 5) * 40)
                   for i in range(64)]
    frames = H.pcap_frames(frames)
    _run_case(tmp_path, prog, frames, mode="direct", cos_pools=1, burst=64)


def test_rx_loop_packets_outside_pinned_arena(built, gpu, tmp_path):
    """Loop packets from a pool in ordinary memory: the GPU staging of the
    loop burst finds them outside the page-locked arena (not_in_place) and
    the host stages (copies), classifies and delivers that burst; the result
    is the reference's."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    _run_case(tmp_path, zoo.prog_everything(), frames, pktio="loop", cos_pools=0, burst=32,
              env_extra={"RX_FEED_POOL": "1", "ODP_AMD_PAGEABLE_POOLS": "feedPool"})


def _ports_prog(nplain, nhash=0, hash_nq=32):
    """A default CoS, `nplain` plain CoS selected by UDP destination port
    5000 + i and `nhash` hash-queue CoS (hash_nq queues, IPv4/UDP hash) by
    port 6000 + j; frames cycle over every port and a miss port."""
    prog = [R.cos("dflt")]
    for i in range(nplain):
        prog.append(R.cos(f"p{i}"))
    for j in range(nhash):
        prog.append(R.cos(f"h{j}", num_queue=hash_nq, hash_proto=R.HP_IPV4_UDP))
    prog.append(("default", 0))
    for i in range(nplain):
        prog.append(("pmr", [R.t_be16(R.PMR_UDP_DPORT, 5000 + i)], 0, 1 + i, 0))
    for j in range(nhash):
        prog.append(("pmr", [R.t_be16(R.PMR_UDP_DPORT, 6000 + j)], 0, 1 + nplain + j, 0))
    ports = [5000 + i for i in range(nplain)] + [6000 + j for j in range(nhash)] + [7]
    frames = [pg.udp4_frame(src=f"10.1.{k % 7}.{k % 251}", sport=1000 + k % 97,
                            dport=ports[k % len(ports)], size=60 + (k * 37) % 400)
              for k in range(3 * 4096 + 123)]
    return prog, frames


@pytest.mark.parametrize("case", ["fits", "pools", "queue_entries"])
def test_rx_chain_table_limits(built, gpu, tmp_path, case):
    """Programs past the receive chain's table limits (include/mi_cls.h:
    MI_CLS_RX_POOLS pool slots, MI_CLS_RX_QENT queue entries; CoS indexes are
    below 256 by the record's u8) leave the chain -- every burst is decided on
    the host -- and are delivered exactly as the reference would
    (rt_helpers.expected), never clamped into the device tables.  `fits`:
    the same shape inside the limits takes the chain."""
    if case == "fits":
        prog, frames = _ports_prog(14)      # pktio pool + 15 CoS pools = 16 slots
        cos_pools, env, shared = 1, {}, None
    elif case == "pools":
        prog, frames = _ports_prog(15)      # 17 pool slots > MI_CLS_RX_POOLS
        cos_pools, env, shared = 1, {}, None
    else:
        # 31 hash CoS x 32 queues + 33 plain CoS sharing one queue: 1025
        # queue entries > MI_CLS_RX_QENT, in 993 queues
        prog, frames = _ports_prog(32, nhash=31)
        cos_pools, env, shared = 0, {"RX_SHARE_QUEUE": "1"}, "shared"
    # (the driver drains its queues after the capture: a shared pktio pool
    # holds every frame)
    env.update(ODP_AMD_RX_BURST="4096", RX_POOL_NUM="6000" if cos_pools else "16384")
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    prof = {}
    got = H.run_driver(f"pcap:in={pc}", rules, "direct", 4, cos_pools, 1, env=env, prof=prof)
    H.compare(got, H.expected(prog, frames, cos_pools, 1, 4, shared_queue=shared))
    assert prof.get("bursts", 0) >= 4, prof
    if case == "fits":
        assert prof["chain_bursts"] >= 1, prof
    else:
        assert prof.get("chain_bursts", 0) == 0 and prof.get("chain_redo", 0) == 0, prof


def test_rx_chain_small_pool(built, gpu, tmp_path):
    """CoS pools of 2600 packets, 1024-frame bursts, the chain on and the
    application draining its queues after every receive call (the driver's
    rate mode): the chain's speculative takes leave a burst's
    worth in each pool, so no allocation fails on packets held only
    speculatively -- every frame is delivered and none is discarded, as the
    reference's sequential receive with the same drain delivers them."""
    prog, frames = _ports_prog(3)
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    prof = {}
    _, stats, _ = H.run_driver(f"pcap:in={pc}", rules, "direct", 4, 1, 1, prof=prof,
                               env={"ODP_AMD_RX_BURST": "1024", "RX_POOL_NUM": "2600",
                                    "RX_COUNT_ONLY": "1"})
    exp = H.expected(prog, frames, 1, 1, 4)[1]
    assert stats == exp, (stats, exp)   # in_packets, in_errors, in_discards (0), octets
    assert prof["chain_bursts"] >= 1, prof


@pytest.mark.parametrize("delivery", list(DELIVERY_ENV))
def test_rx_pool_runs_short(built, gpu, tmp_path, delivery):
    """Every CoS pool (200 packets) is a third of its CoS's traffic and the
    application frees nothing until the capture is through (direct mode drains
    the queues afterwards): on every delivery path each queue receives exactly
    the first 200 packets of its CoS in arrival order -- the frames a
    frame-by-frame odp_packet_alloc would have served -- and every later
    frame is counted in in_discards and leaves in_packets / in_octets
    (pktio/loop.c:332-337, 352-355).  Bursts of 61 do not divide the pool."""
    P = 200
    env = DELIVERY_ENV[delivery]
    prog, frames = _ports_prog(3)   # dflt, p0, p1, p2: one queue and one pool each
    frames = frames[:12 * P]        # 3 P frames per CoS
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    eq, (in_pk, in_err, in_disc, octets), eqs = H.expected(prog, frames, 1, 1, 4)
    assert sorted(eq) == ["dflt", "p0", "p1", "p2"] and all(len(v) == 3 * P for v in eq.values())
    for q, pkts in eq.items():
        assert all(p[0] == q + "Pool" for p in pkts)   # a pool of its own, dflt too
        for p in pkts[P:]:
            in_disc += 1
            if not p[2]:
                in_pk -= 1
                octets -= p[6]
        eq[q] = pkts[:P]
        eqs[(q, 0)] = [P, 0]
    got = H.run_driver(f"pcap:in={pc}", rules, "direct", 4, 1, 1,
                       env=dict(env, ODP_AMD_RX_BURST="61", RX_POOL_NUM=str(P)))
    H.compare(got, (eq, (in_pk, in_err, in_disc, octets), eqs))


def test_rx_loop_no_pipeline(built, gpu, tmp_path):
    """Loop pktio with the receive pipeline off (ODP_AMD_RX_PIPELINE=0,
    ADVICE r5): each burst is staged and classified synchronously by the
    classic path -- never left for a GPU staging step that does not run."""
    frames = H.pcap_frames([f for _, f in zoo.all_frames()])
    for burst in (61, 4096):
        _run_case(tmp_path, zoo.prog_everything(), frames, mode="direct", pktio="loop",
                  burst=burst, env_extra={"ODP_AMD_RX_PIPELINE": "0"})


def test_rx_pcap_runs_specialised_kernel(built, gpu, tmp_path):
    """odp_pktio_start waits for the rules' program-specialised kernel (rule
    load is control plane), so even a short pcap capture is classified by it
    rather than by the generic kernel (451 of 451 launches were
    generic); ODP_AMD_SPEC_WAIT=0 starts without waiting."""
    prog, frames = _ports_prog(3)
    frames = frames[:1500]
    pc = str(tmp_path / "in.pcap")
    H.write_pcap(pc, frames)
    rules = str(tmp_path / "rules.txt")
    H.write_rules(rules, prog)
    prof = {}
    got = H.run_driver(f"pcap:in={pc}", rules, "direct", 4, 1, 1, prof=prof,
                       env={"ODP_AMD_RX_BURST": "256"})
    H.compare(got, H.expected(prog, frames, 1, 1, 4))
    assert prof.get("specialised") == 1, prof
