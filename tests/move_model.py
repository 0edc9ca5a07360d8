"""CPU model of the pool move (mi_cls_pool_move, include/mi_cls.h).

*** TEST INFRASTRUCTURE ***  move() is the header's per-record rule, one
record after the other, on rx_model.meta_line / copy_extent: which packet a
record's frame ends in, the guards that refuse a record, the 64 bytes of the
packet's metadata line and the frame bytes behind it.  It writes nothing: it
returns ent, out and the list of writes, and apply() puts those into an image
of the memory (and opens the unspecified bytes behind a copied frame in a care
mask).  Nothing here is taken from the kernel.

reference_packets() is something else: the reference's receive loop packet by
packet (pktio/loop.c:319-342 with _odp_pktio_packet_to_pool, include/
odp_packet_io_internal.h:352-371), on packets that are Python objects in pools
with free lists; it knows nothing of plans, addresses or lines.
"""
from types import SimpleNamespace

import numpy as np

from tests import enq_model as M
from tests import pool_model as PM
from tests import rx_model as RX

OUT_FIELDS = ("moved", "inplace", "bytes", "refused")


def dst_queue_of(r, table, dst_queue):
    """The odp_queue_t of a record the enqueue table maps (the enqueue plan's
    "delivered" rule), else 0."""
    cos_nq, cos_q0, ent_dst, ndst = table
    if int(r["outcome"]) != M.OUT_ENQ:
        return 0
    cos, queue = int(r["cos"]), int(r["queue"])
    e = int(cos_q0[cos]) + queue
    if queue < int(cos_nq[cos]) and e < M.ENT and int(ent_dst[e]) < ndst:
        return int(dst_queue[int(ent_dst[e])])
    return 0


def in_arena(p, need, arena_lo, arena_bytes):
    """p is a line's address and [p, p + need) lies inside the arena."""
    return p != 0 and p % 64 == 0 and arena_lo <= p and p + need <= arena_lo + arena_bytes


def move(pkts, pkts_bytes, off, lens, res, dec, idx, got, pk, table, dst_queue, input, headroom,
         data_from_meta, arena_lo, arena_bytes, line_at):
    """(ent, out, writes).  pkts: the frames' buffer (uint8, at least pkts_bytes
    long); got / pk: line addresses (pk None: NULL); line_at(addr): the
    META_DTYPE record of the line at addr before the call.  writes: a list of
    (line address, the line's 64 bytes, the frame's bytes or None)."""
    n = len(res)
    ent = np.zeros(n, np.uint64)
    out = dict.fromkeys(OUT_FIELDS, 0)
    writes = []
    for i in range(n):
        fate = int(dec[i]) & 15
        if fate not in (PM.PF_FRESH, PM.PF_INPLACE):
            continue
        ln, o = int(lens[i]), int(off[i])
        own = int(pk[i]) if pk is not None else 0
        ok = o + ln <= pkts_bytes
        if fate == PM.PF_FRESH:
            line = int(got[int(idx[i])]) if int(idx[i]) < len(got) else 0
            ok = ok and int(idx[i]) < len(got) and \
                in_arena(line, data_from_meta + RX.copy_extent(ln), arena_lo, arena_bytes) and \
                (own == 0 or in_arena(own, 64, arena_lo, arena_bytes))
        else:
            line = own
            ok = ok and pk is not None and in_arena(line, 64, arena_lo, arena_bytes)
        if not ok:
            out["refused"] += 1
            continue
        dq = dst_queue_of(res[i], table, dst_queue)
        if fate == PM.PF_FRESH:
            up = int(line_at(own)["user_ptr"]) if own else 0
            text = RX.meta_line(res[i], ln, headroom, dq, input, up)
            frame = np.asarray(pkts[o: o + ln]).copy()
            out["moved"] += 1
            out["bytes"] += ln
        else:
            old = line_at(line)
            text = RX.meta_line(res[i], ln, int(old["data_off"]), dq, input, int(old["user_ptr"]))
            frame = None
            out["inplace"] += 1
        ent[i] = line
        writes.append((line, text, frame))
    return ent, out, writes


def apply(writes, image, base, data_from_meta, care=None):
    """The writes into image (uint8; image[0] is address `base`); care (same
    shape) gets 0 over [len, copy_extent(len)) of every copied frame."""
    for line, text, frame in writes:
        o = line - base
        image[o: o + 64] = np.frombuffer(text, np.uint8)
        if frame is not None:
            d = o + data_from_meta
            image[d: d + len(frame)] = frame
            if care is not None:
                care[d + len(frame): d + RX.copy_extent(len(frame))] = 0


def meta_lines_np(res, lens, data_off, dq, input, user_ptr):
    """rx_model.meta_line for many records at once (layer ALL), as a META_DTYPE
    array; tests/test_pool_move_cpu.py holds the two equal."""
    m = np.zeros(len(res), RX.META_DTYPE)
    m["data_off"], m["len"], m["in_flags"], m["err"] = data_off, lens, res["in_flags"], res["err"]
    m["cos"], m["cls_mark"], m["l3"], m["l4"] = res["cos"], res["mark"], res["l3_offset"], res["l4_offset"]
    m["dst_queue"], m["input"], m["user_ptr"] = dq, input, user_ptr
    return m


def move_np(image, base, pkts_off, off, lens, res, dec, idx, got, table, dst_queue, input, headroom,
            data_from_meta, care):
    """move() and apply() without a loop per record, for batches without own
    packets (pk NULL) in which no record is refused (the caller's business:
    asserted where it is cheap).  image[0] is address `base`; the frames'
    buffer starts at image[pkts_off].  Writes the lines and frames into image,
    opens care behind the frames, returns (ent, out)."""
    n = len(res)
    lens = np.asarray(lens).astype(np.int64)
    fresh = (np.asarray(dec) & 15) == PM.PF_FRESH
    assert not ((np.asarray(dec) & 15) == PM.PF_INPLACE).any()
    f = np.nonzero(fresh)[0]
    assert (np.asarray(idx)[f] < len(got)).all()
    line = np.asarray(got, np.uint64)[np.asarray(idx)[f]].astype(np.int64)
    assert (line % 64 == 0).all() and len(np.unique(line)) == len(line)
    ent = np.zeros(n, np.uint64)
    ent[f] = line
    k, stale = M.keys(res[f], table)
    dq = np.where(k < table[3], np.asarray(dst_queue, np.uint64)[np.minimum(k, max(table[3] - 1, 0))], 0)
    lines = meta_lines_np(res[f], lens[f], headroom, dq, input, 0)
    at = line - base
    image[(at[:, None] + np.arange(64)).reshape(-1)] = lines.view(np.uint8).reshape(-1)
    for ln in np.unique(lens[f]):
        g = f[lens[f] == ln]
        d = ent[g].astype(np.int64) - base + data_from_meta
        s = pkts_off + np.asarray(off).astype(np.int64)[g]
        image[(d[:, None] + np.arange(ln)).reshape(-1)] = image[(s[:, None] + np.arange(ln)).reshape(-1)]
        ext = RX.copy_extent(int(ln)) - int(ln)
        if ext:
            care[(d[:, None] + ln + np.arange(ext)).reshape(-1)] = 0
    return ent, {"moved": len(f), "inplace": 0, "bytes": int(lens[f].sum()), "refused": 0}


# ---- the reference's loop on packet objects --------------------------------
def reference_packets(frames, records, pkt_pool, user_ptr, ptable, free, table, dst_queue, input,
                      headroom):
    """loop.c:319-342 per packet.  frames[i]: the frame's bytes; pkt_pool[i]:
    the pool (slot) the packet it arrived in belongs to, None for a pool that is
    no slot; user_ptr[i]: that packet's user pointer; free[k]: pool k's free
    packets (a list of names, taken from the front).  A packet is delivered
    when the classifier returned 0 and _odp_pktio_packet_to_pool succeeded:
    in its own packet when that is of the CoS's pool already, else in a packet
    allocated from the CoS's pool, into which odp_packet_copy copied the data
    and the metadata (user pointer included; headroom is the pool's).  Returns
    per frame None or a namespace(pool, name (None: its own packet), data,
    len, user_ptr, headroom (None: its own packet's), record fields, dst_queue,
    input)."""
    cos_slot, slot_cap, nslot = ptable
    free = [list(f) for f in free]
    out = []
    for i, r in enumerate(records):
        out.append(None)
        if int(r["outcome"]) != M.OUT_ENQ:        # parse drop, classifier != 0: freed
            continue
        new_pool = int(cos_slot[int(r["cos"])])
        if new_pool >= nslot:                     # not of this control plane
            continue
        ln = len(frames[i])
        if pkt_pool[i] is not None and pkt_pool[i] == new_pool:
            name, hr = None, None                 # new_pool == odp_packet_pool(*pkt)
        else:                                     # odp_packet_copy(*pkt, new_pool)
            if not free[new_pool] or ln > int(slot_cap[new_pool]):
                continue                          # ODP_PACKET_INVALID: freed, in_discards
            name, hr = free[new_pool].pop(0), headroom
        out[i] = SimpleNamespace(pool=new_pool, name=name, data=bytes(frames[i]), len=ln,
                                 user_ptr=int(user_ptr[i]), headroom=hr, in_flags=int(r["in_flags"]),
                                 err=int(r["err"]), cos=int(r["cos"]), mark=int(r["mark"]),
                                 l3=int(r["l3_offset"]), l4=int(r["l4_offset"]),
                                 dst_queue=dst_queue_of(r, table, dst_queue), input=input)
    return out
