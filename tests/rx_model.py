"""CPU model of the receive delivery and the receive chain (include/mi_cls.h,
"Receive delivery on the GPU" and "The receive chain").

*** TEST INFRASTRUCTURE ***  A plain sequential restatement of what the
header specifies and of the reference steps it cites: the receive loops
(pktio/loop.c:308-373, pcap.c:330-352), the pktio's per-packet drop / pool /
counter rules (odp_packet_io.c:680-705), the enqueue runs of _odp_cls_enq
(include/odp_classification_internal.h:142-236) and the parser layers
(odp_parse.c:372-414).  One loop over the frames in arrival order: no waves,
no segments, nothing taken from the kernels.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from odp_amd import rules as R

RESULT_DTYPE = R.RESULT_DTYPE

# mi_cls_pkt_meta_t: the 64-byte metadata line of a packet header
META_DTYPE = np.dtype([("data_off", "<u4"), ("len", "<u4"), ("in_flags", "<u8"), ("err", "u1"),
                       ("cos", "u1"), ("cls_mark", "<u2"), ("l2", "<u2"), ("l3", "<u2"),
                       ("l4", "<u2"), ("rsv0", "<u2"), ("rsv1", "<u4"), ("dst_queue", "<u8"),
                       ("input", "<u8"), ("user_ptr", "<u8"), ("rsv2", "<u8")])
assert META_DTYPE.itemsize == 64

# mi_cls_dlv_t: one delivered packet of mi_cls_deliver_submit
DLV_DTYPE = np.dtype([("meta", "<u8"), ("dst_queue", "<u8"), ("user_ptr", "<u8"), ("src", "<u4"),
                      ("rec", "<u4"), ("len", "<u2"), ("flags", "u1"), ("qid", "u1"),
                      ("data_off", "<u4"), ("rsv", "<u8")])
assert DLV_DTYPE.itemsize == 48

RX_POOLS, RX_QENT, DLV_GROUPS, DLV_GROUP_MAX = 16, 1024, 64, 8192
RXT_CLS, RXT_GROUP = 1, 2
DLV_FRESH, DLV_COPY, DLV_CLS = 1, 2, 4
RXF_DROP, RXF_DISCARD, RXF_FRESH, RXF_INPLACE = 0, 1, 2, 3
NO_GROUP = 0x7F

# mi_cls_rxtab_t
RXTAB_DTYPE = np.dtype([("flags", "<u4"), ("npool", "<u4"), ("pool_cap", "<u4", (RX_POOLS,)),
                        ("rt_slot", "u1", (64,)), ("cos_pool", "u1", (256,)),
                        ("cos_nq", "u1", (256,)), ("cos_q0", "<u2", (256,)),
                        ("rt_pinned", "u1", (64,)), ("qh", "<u8", (RX_QENT,)),
                        ("qg", "u1", (RX_QENT,)), ("stamp", "<u8")], align=True)

# mi_cls_rx_out_t
RXOUT_DTYPE = np.dtype([("in_errors", "<u8"), ("in_discards", "<u8"), ("packets", "<u8"),
                        ("octets", "<u8"), ("used", "<u4", (RX_POOLS,)),
                        ("need", "<u4", (RX_POOLS,)), ("short_pool", "<u4"),
                        ("not_in_place", "<u4"), ("rsv", "<u4", (2,))])

# input_flags bits (include/odp/api/plat/packet_inline_types.h:60-107) by the
# parser step that sets them
_L2_BITS = ("l2", "eth", "eth_bcast", "eth_mcast", "jumbo", "vlan", "vlan_qinq")
_L3_BITS = ("l3", "arp", "ipv4", "ipv6", "ip_bcast", "ip_mcast", "ipfrag", "ipopt",
            "l3_chksum_done")
_BIT = {"cls_mark": 0, "flow_hash": 1, "timestamp": 2, "l2": 3, "l3": 4, "l4": 5, "eth": 6,
        "eth_bcast": 7, "eth_mcast": 8, "jumbo": 9, "vlan": 10, "vlan_qinq": 11, "arp": 12,
        "ipv4": 13, "ipv6": 14, "ip_bcast": 15, "ip_mcast": 16, "ipfrag": 17, "ipopt": 18,
        "l3_chksum_done": 30, "l4_chksum_done": 31}
L2_FLAGS = sum(1 << _BIT[b] for b in _L2_BITS)
L3_FLAGS = L2_FLAGS | sum(1 << _BIT[b] for b in _L3_BITS)
# flags.all.error bits (packet_inline_types.h:152-158): snap_len, ip, l3_chksum
L2_ERR, L3_ERR = 0x01, 0x07


def apply_layer(fl, err, l4, layer):
    """What a parser layer (ODP_PROTO_LAYER_L2..ALL = 1..4) records of the
    full parse: _odp_packet_parse_common_l3_l4 returns before the L3 switch at
    L2 (odp_parse.c:374) and before the L4 switch at L3 (:412), so only the
    flags and errors set up to there exist, and l4_offset is set by the L3
    parsers alone (:387, :397)."""
    if layer >= 3:
        return fl, err, l4
    if layer == 1:
        return fl & L2_FLAGS, err & L2_ERR, 0xFFFF
    return fl & L3_FLAGS, err & L3_ERR, l4


def meta_line(record, length, data_off, dq, input, user_ptr, layer=4, cos=None, mark=None):
    """The 64 bytes of a delivered packet's mi_cls_pkt_meta_t (every rsv
    field zero, l2_offset 0).  cos / mark default to the record's."""
    fl, err, l4 = apply_layer(int(record["in_flags"]), int(record["err"]),
                              int(record["l4_offset"]), layer)
    m = np.zeros((), META_DTYPE)
    m["data_off"], m["len"], m["in_flags"], m["err"] = data_off, length, fl, err
    m["cos"] = int(record["cos"]) if cos is None else cos
    m["cls_mark"] = int(record["mark"]) if mark is None else mark
    m["l3"], m["l4"] = int(record["l3_offset"]), l4
    m["dst_queue"], m["input"], m["user_ptr"] = dq, input, user_ptr
    return m.tobytes()


def copy_extent(length):
    """Bytes of a packet's data area a frame copy may write: the frame goes in
    16-byte pieces, so [0, len) is the frame, [len, round_up(len, 16)) is
    unspecified, and nothing at or beyond round_up(len, 16) is touched.  The
    runtime's packet buffers guarantee it: a pool's data capacity is a
    multiple of 64 (odp_rt.c odp_pool_create: cap = align_up(len, 64)) with
    RT_PKT_TAILROOM behind it, and no frame longer than pool_cap is copied."""
    return (int(length) + 15) & ~15


def stable_groups(qids, limit=DLV_GROUP_MAX):
    """The stable grouping of the entries with a queue group (< 64): perm (entry
    indexes, group by group, arrival order inside a group) and the counts."""
    q = np.asarray(qids[:limit], dtype=np.int64)
    idx = np.nonzero(q < DLV_GROUPS)[0]
    perm = idx[np.argsort(q[idx], kind="stable")].astype(np.uint32)
    cnt = np.bincount(q[idx], minlength=DLV_GROUPS).astype(np.uint32)
    return perm, cnt


def decide(records, lens, tab, have, got_base, got, pk=None, ppool=None):
    """The per-frame decisions of one burst (mi_cls_rx_chain_submit,
    include/mi_cls.h "The receive chain"; odp_packet_io.c:680-705 per frame).
    Fate: a parse drop or a CoS drop is DROP; no CoS (discard, CoS cycle) is
    DISCARD; an enqueued frame whose own packet (loop, pk) is of its CoS's
    pool slot is INPLACE, one longer than the slot's pool_cap DISCARD (the
    allocation fails), any other FRESH with the rank = the earlier FRESH
    frames of its slot.  Delivered: INPLACE, or FRESH with rank < have[slot].
    packets / octets count delivered frames without an error, in_errors the
    frames with an error or a parse drop.  Returns dec, ent, dq (the queue
    handle of a delivered frame), perm, gcnt (count | 1 << 24 | cos << 16 when
    the group's frames all have one CoS) and out."""
    n = len(records)
    flags = int(tab["flags"])
    cap = [int(x) for x in tab["pool_cap"]]
    dec = np.zeros(n, np.uint32)
    ent = np.zeros(n, np.uint64)
    dq = np.zeros(n, np.uint64)
    qid = np.full(n, 0xFF, np.int64)
    delivered = np.zeros(n, bool)
    need = [0] * RX_POOLS
    out = SimpleNamespace(in_errors=0, in_discards=0, packets=0, octets=0, used=[0] * RX_POOLS,
                          need=need, short_pool=0)
    gcos = [set() for _ in range(DLV_GROUPS)]
    for i in range(n):
        r = records[i]
        oc, err, cos, ln = int(r["outcome"]), int(r["err"]), int(r["cos"]), int(lens[i])
        fate, k, rank = RXF_DROP, 0, 0
        if err or oc == R.OUT_PARSE_DROP:
            out.in_errors += 1
        if oc in (R.OUT_DISCARD, R.OUT_LOOP):
            fate = RXF_DISCARD
        elif oc == R.OUT_ENQ:
            k = int(tab["cos_pool"][cos])
            assert k < RX_POOLS
            own = 0
            if pk is not None and int(ppool[i]):
                own = int(tab["rt_slot"][(int(ppool[i]) - 1) & 63])
            if own and own - 1 == k:
                fate = RXF_INPLACE      # loop.c: the packet stays in its pool
            elif ln > cap[k]:
                fate = RXF_DISCARD      # the allocation from the CoS pool fails
            else:
                fate = RXF_FRESH
                rank = need[k]
                need[k] += 1
        if fate == RXF_DISCARD:
            out.in_discards += 1
        g = NO_GROUP
        if fate == RXF_INPLACE or (fate == RXF_FRESH and rank < int(have[k])):
            delivered[i] = True
            ent[i] = int(pk[i]) if fate == RXF_INPLACE else int(got[int(got_base[k]) + rank])
            qe = int(tab["cos_q0"][cos]) + int(r["queue"])
            dq[i] = int(tab["qh"][qe])
            if not err:
                out.packets += 1
                out.octets += ln
            if flags & RXT_GROUP:
                g = int(tab["qg"][qe])
                assert g < DLV_GROUPS
                qid[i] = g
                gcos[g].add(cos)
        assert rank <= 0xFFFF
        dec[i] = fate | (k << 2) | (g << 8) | (rank << 16)
    for k in range(RX_POOLS):
        out.used[k] = min(need[k], int(have[k]))
        out.short_pool |= int(need[k] > int(have[k]))
    perm, cnt = stable_groups(qid)
    gcnt = cnt.copy()
    for g in range(DLV_GROUPS):
        if cnt[g] and len(gcos[g]) == 1:
            gcnt[g] = int(cnt[g]) | (1 << 24) | (next(iter(gcos[g])) << 16)
    return SimpleNamespace(dec=dec, ent=ent, dq=dq, perm=perm, gcnt=gcnt, out=out,
                           delivered=delivered, grouped=bool(flags & RXT_GROUP))


def chain_meta(dcs, i, record, length, headroom, input, old_meta, pk_meta):
    """The metadata line the chain writes for delivered frame i: a fresh
    packet gets the pktio's headroom and, on a pool switch (pk_meta: the
    frame's own packet's line), that packet's user pointer; a packet received
    in place (old_meta: its line before) keeps headroom and user pointer."""
    fate = int(dcs.dec[i]) & 3
    if fate == RXF_INPLACE:
        doff, up = int(old_meta["data_off"]), int(old_meta["user_ptr"])
    else:
        doff, up = headroom, (int(pk_meta["user_ptr"]) if pk_meta is not None else 0)
    return meta_line(record, length, doff, int(dcs.dq[i]), input, up)


def deliver(records, dlv, layer, input, headroom, old_meta):
    """mi_cls_deliver_submit: per entry its metadata line (old_meta[j]: the
    packet's line before, read for entries that are not FRESH), plus the
    stable perm and the plain per-group counts of the first DLV_GROUP_MAX
    entries."""
    lines = []
    for j in range(len(dlv)):
        d = dlv[j]
        r = records[int(d["rec"])]
        fl = int(d["flags"])
        fresh, cls = bool(fl & DLV_FRESH), bool(fl & DLV_CLS)
        if cls:       # _odp_cls_classify_packet's fields
            cos, mark, dq = int(r["cos"]), int(r["mark"]), int(d["dst_queue"])
        elif fresh:   # packet_parse_reset's: none
            cos, mark, dq = 0xFF, 0, 0
        else:         # parser-only pktio, the packet as it was sent
            o = old_meta[j]
            cos, mark, dq = int(o["cos"]), int(o["cls_mark"]), int(o["dst_queue"])
        lines.append(meta_line(r, int(d["len"]), headroom if fresh else int(d["data_off"]), dq,
                               input, 0 if fresh else int(d["user_ptr"]), layer, cos, mark))
    perm, gcnt = stable_groups(dlv["qid"])
    return SimpleNamespace(lines=lines, perm=perm, gcnt=gcnt)


def stage(headers, base, nbytes, rt_pinned):
    """Loop staging (args.stage): headers[i] = (head, pool, data_off, len) of
    frame i's packet.  A descriptor is kept when the pool is a page-locked
    one and the data (with the 16-byte read slack) lies inside
    [base, base + nbytes)."""
    n = len(headers)
    soff, slen, ppool = np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    nip = 0
    for i, (head, pool, doff, ln) in enumerate(headers):
        da, ln = int(head) + int(doff), min(int(ln), 65535)
        ok = pool < 64 and bool(rt_pinned[pool]) and base <= da <= base + nbytes - ln - 16
        ppool[i] = (pool + 1) & 0xFF
        if ok:
            soff[i], slen[i] = da - base, ln
        else:
            nip = 1
    return SimpleNamespace(soff=soff, slen=slen, ppool=ppool, not_in_place=nip)


def queues_of(dcs, n):
    """Per destination queue handle the frames it receives, in order: the
    groups of perm in turn (gcnt bits 0-15), or arrival order when the table
    does not group."""
    order = []
    if dcs.grouped:
        at = 0
        for g in range(DLV_GROUPS):
            c = int(dcs.gcnt[g]) & 0xFFFF
            order += [int(x) for x in dcs.perm[at: at + c]]
            at += c
        assert at == len(dcs.perm)
    else:
        order = [i for i in range(n) if dcs.delivered[i]]
    q = {}
    for i in order:
        q.setdefault(int(dcs.dq[i]), []).append(i)
    return q


def prog_table(prog, cos_pools, group=True, cap=1856):
    """A receive-chain table for a rule program as the runtime's control plane
    lays it out: CoS index -> pool slot (slot 0 the pktio's pool, a pool per
    CoS with cos_pools), its queues' handles and groups (queue entry modulo
    64: several queues may share a group).  Returns (table, pool names by
    slot, queue names by handle)."""
    from tests.rt_helpers import cos_names
    tab = np.zeros((), RXTAB_DTYPE)
    tab["flags"] = RXT_CLS | (RXT_GROUP if group else 0)
    pools, qnames, qe = ["pktio_pool"], {}, 0
    for idx, (name, a) in sorted(cos_names(prog).items()):
        if a["action"] == 1:
            continue
        pool = name[:24] + "Pool" if cos_pools else "pktio_pool"
        if pool not in pools:
            pools.append(pool)
        tab["cos_pool"][idx] = pools.index(pool)
        tab["cos_nq"][idx] = a["num_queue"]
        tab["cos_q0"][idx] = qe
        for s in range(a["num_queue"]):
            h = 0x7000_0000_0000 + 64 * qe
            tab["qh"][qe], tab["qg"][qe] = h, qe % DLV_GROUPS
            qnames[h] = name if a["num_queue"] == 1 else f"_odp_cos_hq_{idx}_{s}"
            qe += 1
    assert len(pools) <= RX_POOLS and qe <= RX_QENT
    tab["npool"] = len(pools)
    tab["pool_cap"][:] = cap
    tab["stamp"] = 1
    return tab, pools, qnames
