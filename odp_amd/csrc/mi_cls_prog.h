// mi_cls_prog.h -- the device rule-program encoding: the words the host
// assembler (mi_cls_asm.cpp) writes and the kernels (mi_cls_dev.h) follow
// without checking.  Layout constants, the field descriptors of the term
// kinds and the two cuckoo hash functions, each defined once for both sides.
// Plain C++17: compiles under g++, hipcc and hipRTC.
#pragma once
#include <stdint.h>

#include "mi_cls.h"

// host/device qualifier of the functions both sides call (empty for plain C++)
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define MI_HD __host__ __device__
#else
#define MI_HD
#endif

// ---------------------------------------------------------------- flags
// input_flags bits: include/odp/api/plat/packet_inline_types.h:66-107
#define F_CLS_MARK  (1u << 0)
#define F_L2        (1u << 3)
#define F_L3        (1u << 4)
#define F_L4        (1u << 5)
#define F_ETH       (1u << 6)
#define F_ETH_BCAST (1u << 7)
#define F_ETH_MCAST (1u << 8)
#define F_JUMBO     (1u << 9)
#define F_VLAN      (1u << 10)
#define F_QINQ      (1u << 11)
#define F_ARP       (1u << 12)
#define F_IPV4      (1u << 13)
#define F_IPV6      (1u << 14)
#define F_IP_BCAST  (1u << 15)
#define F_IP_MCAST  (1u << 16)
#define F_IPFRAG    (1u << 17)
#define F_IPOPT     (1u << 18)
#define F_IPSEC     (1u << 19)
#define F_AH        (1u << 20)
#define F_ESP       (1u << 21)
#define F_UDP       (1u << 22)
#define F_TCP       (1u << 23)
#define F_SCTP      (1u << 24)
#define F_ICMP      (1u << 25)
#define F_NO_NEXT   (1u << 26)

// ------------------------------------------------------ field descriptors
// Where the key words of a term kind sit (verify_pmr_<term>,
// odp_classification.c:931-1357): 4-byte little-endian words at
// base + add, or base + alt when the lane's flags have `altf`
// (QinQ outer tag, IPv4 vs IPv6 next-header, AH vs ESP SPI); base is the
// frame start, L3 or L4.  The term's mask words cut each word down to the
// field (e.g. 0xffff for a 16-bit field), so every kind but LEN, PCP and
// DSCP is "read words, AND mask".  gate: the packet has the field iff its
// flags share a bit with `gate` (~0: always).  The verifiers' presence tests
// map onto single flag masks: eth && vlan is F_VLAN (both parsers set VLAN
// only on frames that keep F_ETH), vlan || qinq, ipv4 || ipv6, ah || esp;
// "l2 && l3 valid" (custom L3) is F_L2 plus the l3 != invalid test in
// field_off.
enum { FB_FRAME = 0, FB_L3 = 1, FB_L4 = 2 };
// classification-block pseudo kind: UDP and TCP port terms with one mask
// (class_of), the raw port word at l4 tagged with the protocol
#define K_L4PORT 0x40u
struct FDesc {
	uint32_t base, add, alt, altf, gate;
};

MI_HD inline FDesc fdesc(uint32_t kind, uint32_t toff)
{
	FDesc d = { FB_FRAME, 0u, 0u, 0u, 0u };
	switch (kind) {
	case MI_K_ETH0: d = { FB_FRAME, 12u, 12u, 0u, F_ETH }; break;
	case MI_K_ETHX: d = { FB_FRAME, 16u, 20u, F_QINQ, F_VLAN | F_QINQ }; break;
	case MI_K_VID0: d = { FB_FRAME, 14u, 14u, 0u, F_VLAN }; break;
	case MI_K_VIDX: d = { FB_FRAME, 14u, 18u, F_QINQ, F_VLAN | F_QINQ }; break;
	case MI_K_DMAC: d = { FB_FRAME, 0u, 0u, 0u, F_ETH }; break;
	case MI_K_PROTO: d = { FB_L3, 6u, 9u, F_IPV4, F_IPV4 | F_IPV6 }; break;
	case MI_K_UDP_DPORT:
	case MI_K_UDP_SPORT: d = { FB_L4, 0u, 0u, 0u, F_UDP }; break;
	case MI_K_TCP_DPORT:
	case MI_K_TCP_SPORT: d = { FB_L4, 0u, 0u, 0u, F_TCP }; break;
	case K_L4PORT: d = { FB_L4, 0u, 0u, 0u, F_UDP | F_TCP }; break;
	case MI_K_SIP: d = { FB_L3, 12u, 12u, 0u, F_IPV4 }; break;
	case MI_K_DIP: d = { FB_L3, 16u, 16u, 0u, F_IPV4 }; break;
	case MI_K_SIP6: d = { FB_L3, 8u, 8u, 0u, F_IPV6 }; break;
	case MI_K_DIP6: d = { FB_L3, 24u, 24u, 0u, F_IPV6 }; break;
	case MI_K_SPI: d = { FB_L4, 0u, 4u, F_AH, F_AH | F_ESP }; break;
	case MI_K_CUSTOM_FRAME: d = { FB_FRAME, toff, toff, 0u, ~0u }; break;
	case MI_K_CUSTOM_L3: d = { FB_L3, toff, toff, 0u, F_L2 }; break;
	default: break;
	}
	return d;
}

// ------------------------------------------------------ device rule program
// mi_cls_rules_load() assembles the mi_cls.h table into this private,
// read-only encoding (32-bit words):
//
//   [0, 16)              header (DH_* below)
//   [hot_off, +hot_words)  HOT region -- everything a lane may look up with its
//                        own (per-lane) index.  All offsets inside it are
//                        relative to hot_off, so the kernel can read it from
//                        HBM or from a copy in LDS with the same indices:
//      CoS table        4 words per CoS slot: #rules, bit-vector block (0 =
//                       linear scan), meta = action | num_queue<<8 |
//                       hash_proto<<16 | index<<24, first rule record
//      BV blocks        see below
//   [prog_off, ...)      COLD region -- 16-word rule records, read only with
//                        wave-uniform (scalar) loads by the linear engine:
//        w0  = inline terms | ext terms<<8 | mark<<16
//        w1  = dst CoS | ext word offset<<8
//        w2.. terms: op word (kind | size<<8 | nw<<16), [offset word for custom
//             kinds], then nw (mask, value) word pairs; terms that do not fit
//             the 14 inline words continue at the ext offset.
enum { DH_MAGIC = 0, DH_NCOS, DH_DEFAULT, DH_ERROR, DH_DEFAULT_VALID, DH_USED, DH_MAX_HOPS,
       DH_HOT_OFF, DH_PROG_OFF, DH_TOTAL, DH_HOT_WORDS,
       // furthest byte past L3 / L4 / the frame start any term (or the hash
       // queue tuple) of the program reads: the kernel's window predictor
       DH_L3END, DH_L4END, DH_FREND,
       // hot-region word of the joint groups' directory (0: none)
       DH_JOINT, DH_WORDS = 16 };
#define DEV_MAGIC 0x33564544u   // "DEV3"
#define REC_WORDS 16u
#define COS_WORDS 4u
#define C_NR 0u
#define C_BV 1u
#define C_META 2u
#define C_REC0 3u
#define BV_MAX_CLS 8u
#define BV_CLS_WORDS 16u
#define BV_WIDE_WORDS 8u        // wide bitmap rows: up to 256 rules
// class words 14-15: the field descriptor of the class's kind (fdesc()),
// resolved at rule load so the device decodes it instead of switching on
// kind: w14 = add | alt << 16; w15 = gate (flag mask, bits 0-23) | base << 24
// | alt-flag code << 26 (1 QinQ, 2 IPv4, 3 AH) | BVF_* << 28
#define BVC_AO 14u
#define BVC_DESC 15u
#define BVF_SPECIAL 1u          // LEN / PCP / DSCP: special_value()
#define BVF_CUSTOM 2u           // custom frame / L3: length test
#define BVF_L3 4u               // custom L3: l3 must be valid
#define BVF_TAG 8u              // merged UDP/TCP port class: protocol tag at bit cr(3)
#define BV_EMPTY 0xFFFFFFFFu
#define BV_NONE 0xFFFFFFFEu
// direct blocks: a slot value / miss word is the rule's result word
// (dst | leaf << 8 | mark << 16) with this bit set; 0 / BV_EMPTY: no rule
#define BV_RES_VALID 0x200u
// joint tables (tree programs): direct blocks sharing a class record, and
// bitmap blocks over the same class records, probe one table per class over
// (key, CoS); header word 1 of a direct member block, word 13 of a bitmap
// member's class record (and word 6 of the class's info in the group's
// info) say how the CoS slot enters the key: in 8 bits of a one-word key no
// rule can set (at bit BVJ_SHIFT's value), or appended as the last key word.
// Group info (hc[DH_JOINT + group - 1] = its word): kind (0 direct, 2
// bitmap), #classes, alive rows and result-array words per CoS slot
// (bitmap), then 8 words per class: class record, #buckets, table, m1, m2,
// miss values per CoS slot, BVJ flags
#define BVJ_ONEWORD 0x10000u
#define BVJ_APPEND 0x20000u
#define BVJ_SHIFT 18u
// CoS entry word C_BV: block offset (bits 0-23), joint group + 1 (bits
// 24-30, tree programs), chain of blocks (bit 31, flat programs)
#define C_BV_OFF 0xFFFFFFu

// Classification block of a CoS ("BV" block for historical reasons), used
// when its rules fall into at most BV_MAX_CLS key classes (a key class is one
// (term kind, mask[, offset, size]) combination).  build_bv() explains the
// modes; the layout (word indices into the hot region) is:
//   b[0] mode (0 direct, 1 candidate, 2 bitmap, 3 wide bitmap, 4 single
//   candidate), b[1] #classes, b[2] result words (dst | leaf<<8 | mark<<16
//   per rule; leaf = the destination CoS has no rules, so the descent ends
//   there), b[3] first rule without a classified term (BV_NONE: none), b[4]
//   rule records (bitmap: alive row; wide: block-relative index of the
//   nw-word alive row), b[5] record words, b[6] wide: nw = words per row
//   class record (16 words): kind, nkey, miss value (wide: index of the miss
//                   row), offset (custom) / tag bit (merged ports), size,
//                   mask[4], #buckets, table offset, cuckoo multipliers m1,
//                   m2, list base, field descriptor (BVC_AO, BVC_DESC)
//   modes 1-4: class k's record at b[8 + 16 k]
//   direct blocks (mode 0, split class): the record holds only what the
//                   class is and is shared by every direct block with that
//                   class; the block keeps the 6-word class info in b[2..7]:
//                   shared record index, miss word, #buckets, table offset,
//                   m1, m2 (no results array)
//   table (16-B aligned): one-word keys 2 slots of (key, value) per 16-B
//             bucket; 2-3-word keys one 16-B slot (key words, value);
//             4-word keys one 32-B slot; value 0: empty
//     direct: the result word of the first live rule with this key or
//             without a term of the class, | BV_RES_VALID (BV_EMPTY: none)
//     bitmap: the 32-bit row of rules with this key or without a term
//     wide:   index of the nw-word row of rules with this key or without a
//             term of the class (rows are deduplicated)
//     candidate: key id | list length << 12 | list offset << 20; the list
//             holds the rules filed under this key, in scan order
//     single candidate: key id << 16 | 1 + the rule filed under the key
//   rule record (candidate, 1 + ceil(#classes / 2) words): constrained-
//             class mask (bit 31: never holds), then the required key id of
//             class c in half c & 1 of word 1 + c / 2
//   rule record (single candidate, 4 or 8 words): constrained-class mask,
//             then the required value (key id for longer keys) per class,
//             or (compact, 4 words) of the <= 3 constrained classes in order

// Engine value of a program-specialised kernel whose default CoS has a chain
// of blocks (flat programs only): the blocks, their offsets and engines are
// the spec's constants (S::nblk, S::boff, S::bmode).
#define FM_CHAIN 5

// Fold of a longer key's words to the one word bv_bucket() takes.
MI_HD inline __attribute__((always_inline)) uint32_t bv_fold(const uint32_t k[4])
{
	uint32_t h = k[0] * 0x9E3779B1u ^ k[1] * 0x85EBCA77u ^ k[2] * 0xC2B2AE3Du ^ k[3] * 0x27D4EB2Fu;
	return h ^ (h >> 15);
}

// Cuckoo bucket of a key: x = the key word (one-word keys) or bv_fold (longer
// keys), folded to 24 bits that depend on every key bit, times a 24-bit
// multiplier; bits 8-23 of the product, scaled to [0, nb) (nb <= 65536).
// (The product's top bits stay near zero for small keys -- DSCP, IP
// protocol, small ports -- which then crowd a few buckets; bits 8-23 spread
// any key set.)  Two v_mul_u32_u24 (full rate, unlike a 32-bit multiply).
// The host pass is the same arithmetic, masked to 24 bits in 64-bit products.
MI_HD inline __attribute__((always_inline)) uint32_t bv_bucket(uint32_t x, uint32_t m, uint32_t nb)
{
#ifdef __HIP_DEVICE_COMPILE__
	// (__umul24 returns int: shift the unsigned products)
	const uint32_t h = (uint32_t)__umul24(x ^ (x >> 16), m);
	return (uint32_t)__umul24((h >> 8) & 0xffffu, nb) >> 16;
#else
	const uint32_t y = (x ^ (x >> 16)) & 0xFFFFFFu;
	const uint32_t h = (uint32_t)(y * (uint64_t)(m & 0xFFFFFFu));
	return (uint32_t)(((uint64_t)((h >> 8) & 0xFFFFu) * nb) >> 16);
#endif
}
