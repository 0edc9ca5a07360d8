// mi_cls_asm.cpp -- the rule-program assembler: validates a mi_cls.h table
// and assembles it into the device encoding of mi_cls_prog.h (the words
// every kernel follows without checking), works out which kernels the
// program runs (tree, flat engine, tree plan) and writes the source text of
// its program-specialised kernel.  Host-only C++17: no HIP, no device.
#include "mi_cls_asm.h"

#include "mi_cls.h"
#include "mi_cls_prog.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <set>

MiAsmKnobs mi_asm_knobs_from_env()
{
	MiAsmKnobs k;
	k.no_bv = getenv("MI_CLS_NO_BV") != nullptr;
	k.no_joint = getenv("MI_CLS_NO_JOINT") != nullptr;
	k.no_wide = getenv("MI_CLS_NO_WIDE") != nullptr;
	k.no_cand1 = getenv("MI_CLS_NO_CAND1") != nullptr;
	k.no_portmerge = getenv("MI_CLS_NO_PORTMERGE") != nullptr;
	k.no_flat = getenv("MI_CLS_NO_FLAT") != nullptr;
	k.no_plan = getenv("MI_CLS_NO_PLAN") != nullptr;
	k.verbose = getenv("MI_CLS_VERBOSE") != nullptr;
	const char *e = getenv("MI_CLS_DIV");
	k.div = e ? (atoi(e) != 0) : -1;
	return k;
}

// The sections of a table (validated, or about to be: validate_tbl checks
// the header before it looks at them)
struct Tbl {
	const mi_tbl_hdr_t *h;
	const mi_cos_t *cs;
	const mi_rule_t *rs;
	const mi_term_t *ts;
	explicit Tbl(const void *tbl) : h((const mi_tbl_hdr_t *)tbl)
	{
		const uint8_t *b = (const uint8_t *)tbl;
		cs = (const mi_cos_t *)(b + h->cos_off);
		rs = (const mi_rule_t *)(b + h->rule_off);
		ts = (const mi_term_t *)(b + h->term_off);
	}
};

static int validate_tbl(const void *tbl, size_t bytes)
{
	if (!tbl || bytes < sizeof(mi_tbl_hdr_t))
		return -EINVAL;
	const mi_tbl_hdr_t *h = (const mi_tbl_hdr_t *)tbl;
	if (h->magic != MI_CLS_TBL_MAGIC || h->version != MI_CLS_TBL_VERSION || h->total_bytes != bytes)
		return -EINVAL;
	if (h->num_cos > 256 || h->cos_off != sizeof(mi_tbl_hdr_t))
		return -EINVAL;
	if ((uint64_t)h->rule_off != (uint64_t)h->cos_off + (uint64_t)h->num_cos * sizeof(mi_cos_t) ||
	    (uint64_t)h->term_off != (uint64_t)h->rule_off + (uint64_t)h->num_rules * sizeof(mi_rule_t) ||
	    (uint64_t)h->total_bytes != (uint64_t)h->term_off + (uint64_t)h->num_terms * sizeof(mi_term_t))
		return -EINVAL;
	if (h->default_cos >= (int32_t)h->num_cos || h->error_cos >= (int32_t)h->num_cos ||
	    h->default_cos < -1 || h->error_cos < -1)
		return -EINVAL;
	// every index the kernel follows must stay inside the table
	const Tbl t(tbl);
	for (uint32_t i = 0; i < h->num_cos; ++i) {
		if ((uint64_t)t.cs[i].rule_begin + t.cs[i].num_rules > h->num_rules)
			return -EINVAL;
		if (t.cs[i].num_queue < 1 || t.cs[i].num_queue > 32)
			return -EINVAL;
	}
	for (uint32_t i = 0; i < h->num_rules; ++i) {
		if (t.rs[i].dst_cos >= h->num_cos || t.rs[i].num_terms > 8 ||
		    (uint64_t)t.rs[i].term_begin + t.rs[i].num_terms > h->num_terms)
			return -EINVAL;
	}
	for (uint32_t i = 0; i < h->num_terms; ++i) {
		if (t.ts[i].kind >= MI_K_COUNT || t.ts[i].size > 16)
			return -EINVAL;
	}
	return 0;
}

// Mask word i of a term as the kernel applies it: the term's mask cut down
// to the field's own bits in the 4-byte word the kernel reads (the kernel
// reads every fixed field as a whole little-endian word, see fdesc()).
static uint32_t eff_mask(const mi_term_t &t, uint32_t i)
{
	switch (t.kind) {
	case MI_K_ETH0:
	case MI_K_ETHX:
		return t.mask[i] & 0xffffu;
	case MI_K_VID0:
	case MI_K_VIDX:
		return t.mask[i] & 0xff0fu;      // VLAN ID bits of the raw TCI
	case MI_K_PROTO:
		return t.mask[i] & 0xffu;
	case MI_K_DMAC:
		return i == 1 ? (t.mask[i] & 0xffffu) : t.mask[i];
	default:
		return t.mask[i];
	}
}

// key words a term kind reads
static uint32_t kind_words(uint32_t kind, uint32_t size)
{
	if (kind == MI_K_CUSTOM_FRAME || kind == MI_K_CUSTOM_L3)
		return (size + 3u) / 4u;
	return (kind == MI_K_SIP6 || kind == MI_K_DIP6) ? 4u : (kind == MI_K_DMAC ? 2u : 1u);
}

// words of one term in the device encoding (see "device rule program")
static uint32_t encode_term(const mi_term_t &t, uint32_t *w)
{
	const bool custom = t.kind == MI_K_CUSTOM_FRAME || t.kind == MI_K_CUSTOM_L3;
	const uint32_t nw = kind_words(t.kind, t.size);
	uint32_t n = 0;
	w[n++] = t.kind | ((uint32_t)t.size << 8) | (nw << 16);
	if (custom)
		w[n++] = t.offset;
	for (uint32_t i = 0; i < nw; ++i) {
		w[n++] = eff_mask(t, i);   // (custom kinds: the mask as it is)
		w[n++] = t.value[i];
	}
	return n;
}

// ---- bit-vector block construction (host) ----
struct ClassKey {
	uint32_t kind, nkey, offset, size, mask[4];
	bool operator<(const ClassKey &o) const
	{
		if (kind != o.kind) return kind < o.kind;
		if (offset != o.offset) return offset < o.offset;
		if (size != o.size) return size < o.size;
		for (int i = 0; i < 4; ++i)
			if (mask[i] != o.mask[i]) return mask[i] < o.mask[i];
		return false;
	}
};

typedef std::array<uint32_t, 4> Key4;
typedef std::array<uint32_t, 16> Rec16;   // a class record
// a direct block's split class records: (block word to patch, record)
typedef std::vector<std::pair<uint32_t, Rec16>> SharedRecs;

// Two-choice cuckoo table over `keys`: every key sits in a slot of bucket
// b1 or b2 (a lookup reads both buckets at once, no probe loop).  bsz slots
// per bucket: 2 for one-word keys (a 16-B bucket, load <= 87.5 %), 1 for
// longer keys (load <= 45 %).  Returns the slot (bucket * bsz + j) of every
// key, the bucket count and the multipliers used.
static bool cuckoo_place(const std::vector<Key4> &keys, uint32_t nk, uint32_t bsz, uint32_t &nb_out,
			 uint32_t &m1, uint32_t &m2, std::vector<uint32_t> &slot_of)
{
	const uint32_t n = (uint32_t)keys.size();
	std::vector<uint32_t> fold(n), b1(n), b2(n);   // b1, b2: a key's two buckets under m1, m2
	for (uint32_t i = 0; i < n; ++i)
		fold[i] = nk == 1 ? keys[i][0] : bv_fold(keys[i].data());
	// load <= 87.5 % with 2-slot buckets (below the ~89.7 % two-choice
	// threshold; a failed placement grows the table), <= 45 % otherwise
	uint32_t nb = bsz == 2 ? (n * 4 + 6) / 7 : (n * 20 + 8) / 9 + 1;
	if (nb < 1)
		nb = 1;
	uint64_t rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)n << 17);
	for (int grow = 0; grow < 8 && nb <= 65536u; ++grow, nb += nb / 8 + 1) {
		nb_out = nb;
		for (int attempt = 0; attempt < 64; ++attempt) {
			rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
			m1 = ((uint32_t)rng & 0xFFFFFFu) | 1u;
			rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
			m2 = ((uint32_t)(rng >> 32) & 0xFFFFFFu) | 1u;
			std::vector<int32_t> occ((size_t)nb * bsz, -1);
			slot_of.assign(n, 0);
			for (uint32_t i = 0; i < n; ++i) {
				b1[i] = bv_bucket(fold[i], m1, nb);
				b2[i] = bv_bucket(fold[i], m2, nb);
			}
			bool ok = true;
			for (uint32_t i = 0; i < n && ok; ++i) {
				uint32_t cur = i, b = b1[i];
				for (int kick = 0;; ++kick) {
					// a free slot in either bucket of `cur`
					int32_t fs = -1;
					for (uint32_t bb : { b1[cur], b2[cur] })
						for (uint32_t j = 0; j < bsz && fs < 0; ++j)
							if (occ[(size_t)bb * bsz + j] < 0)
								fs = (int32_t)(bb * bsz + j);
					if (fs >= 0) {
						occ[fs] = (int32_t)cur;
						slot_of[cur] = (uint32_t)fs;
						break;
					}
					if (kick > 500) {
						ok = false;
						break;
					}
					// evict a pseudo-random slot of bucket b (alternating buckets;
					// bsz is 1 or 2, so the mask is rng % bsz without the divide)
					rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
					const uint32_t sl = b * bsz + (uint32_t)(rng & (bsz - 1u));
					const uint32_t ev = (uint32_t)occ[sl];
					occ[sl] = (int32_t)cur;
					slot_of[cur] = sl;
					cur = ev;
					b = b1[ev] == b ? b2[ev] : b1[ev];
				}
			}
			if (ok) {
				// every key must sit in one of its two buckets
				for (uint32_t i = 0; i < n && ok; ++i) {
					const uint32_t bk = slot_of[i] / bsz;
					ok = occ[slot_of[i]] == (int32_t)i &&
					     (bk == bv_bucket(fold[i], m1, nb) ||
					      bk == bv_bucket(fold[i], m2, nb));
				}
				if (ok)
					return true;
				fprintf(stderr, "mi_cls: cuckoo placement self-check failed\n");
			}
		}
	}
	return false;
}

static bool class_of(const MiAsmKnobs &kn, const mi_term_t &t, ClassKey &ck)
{
	memset(&ck, 0, sizeof(ck));
	ck.kind = t.kind;
	switch (t.kind) {
	case MI_K_NEVER:
	case MI_K_ALWAYS:
		return false;
	case MI_K_CUSTOM_FRAME:
	case MI_K_CUSTOM_L3:
		ck.offset = t.offset;
		ck.size = t.size;
		ck.nkey = t.size > 8 ? 4 : (t.size > 4 ? 2 : 1);
		break;
	case MI_K_SIP6:
	case MI_K_DIP6:
		ck.nkey = 4;
		break;
	case MI_K_DMAC:
		ck.nkey = 2;
		break;
	default:
		ck.nkey = 1;
	}
	for (uint32_t i = 0; i < 4; ++i)
		ck.mask[i] = i < ck.nkey ? eff_mask(t, i) : 0;
	// trailing key words the mask clears are not part of the key (an IPv6
	// /64 prefix is a two-word key: half the key reads, 16-B table slots)
	while (ck.nkey > 1 && ck.mask[ck.nkey - 1] == 0)
		--ck.nkey;
	// UDP and TCP port terms read the same bytes (the raw port word at l4)
	// under different gates: one class for both, the protocol carried in
	// two key bits the mask leaves free (tag 1 UDP, 2 TCP; port masks are
	// <= 16 bits, so bits tp, tp+1 exist), so a packet's key holds its
	// protocol and one lookup serves rules of either kind.
	if (!kn.no_portmerge && (t.kind == MI_K_UDP_DPORT || t.kind == MI_K_TCP_DPORT ||
			  t.kind == MI_K_UDP_SPORT || t.kind == MI_K_TCP_SPORT)) {
		uint32_t tp = 0;
		while (tp < 31 && ((ck.mask[0] >> tp) & 3u))
			++tp;
		if (tp < 31) {
			ck.kind = K_L4PORT;
			ck.offset = tp;
		}
	}
	return true;
}

// value words a term requires of its class (the tag of a merged port class)
static Key4 class_value(const mi_term_t &t, const ClassKey &ck)
{
	Key4 v = { 0, 0, 0, 0 };
	for (uint32_t i = 0; i < ck.nkey; ++i)
		v[i] = t.value[i];
	if (ck.kind == K_L4PORT)
		v[0] |= (t.kind == MI_K_UDP_DPORT || t.kind == MI_K_UDP_SPORT ? 1u : 2u) << ck.offset;
	return v;
}

// Build the classification block of one CoS into `blk` (word offsets are
// relative to the start of the hot region; base = blk's first word index).
// Returns false when the CoS needs more than BV_MAX_CLS key classes or its
// candidate lists degenerate (the linear scan is used instead).
//
// Semantics (match_pmr_cos, odp_classification.c:1624-1667): the CoS's
// result is the FIRST rule in scan order all of whose terms hold.  A rule's
// terms are grouped by key class (term kind + mask [+ offset, size]); a rule
// holds iff for every class it constrains the packet has the field and the
// masked field equals the rule's value (two terms of one class with
// different values, or an LD_VNI term, make it unmatchable -- not "alive").
// Every class has a cuckoo table keyed by the values its rules require; a
// packet's lookup (absent field = miss) selects:
//  * DIRECT mode (one class): the first alive rule among "rules with this
//    key or without a term of the class" (stored as 1 + rule); a miss takes
//    the first alive rule without a term of the class.
//  * BITMAP mode (<= 32 rules): the 32-bit row "rules with this key or
//    without a term of the class"; a miss takes the row of the latter.  The
//    AND of the rows with the alive row has the first holding rule as its
//    lowest set bit.
//  * CANDIDATE mode: every distinct (class, value) has a key id (1..); the
//    lookup gives the packet's key id (0: miss).  Every constraining rule is
//    filed under ONE of its classes -- its "primary", the one whose value
//    the fewest rules share -- in a list per key id in scan order.  The
//    candidates are the lists of the packet's key ids plus the first rule
//    with no classified term (it matches everything); a candidate holds iff
//    its record's key ids equal the packet's, and the smallest one wins.
//
// member (a block of a chain, see bv_eval): only the rules it marks are
// alive in this block (the others hold in another block of the chain), the
// numbering stays the CoS's, and the direct engine is not used (a chain
// compares rule numbers across blocks).
// why build_bv gave up (MI_CLS_VERBOSE): the linear scan is used instead
static bool bv_fail(const MiAsmKnobs &kn, int why)
{
	if (kn.verbose)
		fprintf(stderr, "mi_cls: no classification block (reason %d)\n", why);
	return false;
}

// A block's keys and table values per class (direct: result words, bitmap:
// rule rows), for joint tables.
typedef std::vector<std::pair<Key4, uint32_t>> DirectKV;
typedef std::vector<DirectKV> BlockKV;

static bool build_bv(const MiAsmKnobs &kn, const mi_cos_t *cs, const mi_rule_t *rs, const mi_term_t *ts, uint32_t nrules,
		     uint32_t base, std::vector<uint32_t> &blk,
		     SharedRecs &shared,
		     const std::vector<uint8_t> *member = nullptr, BlockKV *bkv = nullptr)
{
	std::map<ClassKey, uint32_t> cls;
	std::vector<ClassKey> cls_list;
	for (uint32_t r = 0; r < nrules; ++r)
		for (uint32_t t = 0; t < rs[r].num_terms && (!member || (*member)[r]); ++t) {
			ClassKey ck;
			if (class_of(kn, ts[rs[r].term_begin + t], ck) && !cls.count(ck)) {
				cls[ck] = (uint32_t)cls_list.size();
				cls_list.push_back(ck);
			}
		}
	const uint32_t ncls = (uint32_t)cls_list.size();
	if (ncls > BV_MAX_CLS || ncls == 0)
		return bv_fail(kn, 1);
	// canonical class order: CoS with the same classes evaluate them in the
	// same order, so lanes on different CoS stay convergent
	std::sort(cls_list.begin(), cls_list.end());
	for (uint32_t i = 0; i < ncls; ++i)
		cls[cls_list[i]] = i;
	// per rule: alive, constrained classes and their values
	std::vector<uint8_t> alive(nrules, 0);
	std::vector<uint32_t> tmask(nrules, 0);
	std::vector<std::vector<Key4>> want(nrules, std::vector<Key4>(ncls));
	std::vector<std::map<Key4, uint32_t>> freq(ncls);   // value -> #alive rules
	for (uint32_t r = 0; r < nrules; ++r) {
		bool ok = !member || (*member)[r];
		for (uint32_t t = 0; t < rs[r].num_terms && ok; ++t) {
			const mi_term_t &tm = ts[rs[r].term_begin + t];
			ClassKey ck;
			if (!class_of(kn, tm, ck)) {
				if (tm.kind == MI_K_NEVER)
					ok = false;
				continue;
			}
			const uint32_t c = cls[ck];
			const Key4 v = class_value(tm, ck);
			// a value bit under a zero mask word (trimmed from the key) can
			// never be matched; values are pre-masked by the control plane,
			// this guards other producers of the table
			for (uint32_t i = ck.nkey; i < 4; ++i)
				if ((kind_words(tm.kind, tm.size) > i) && tm.value[i] != 0u)
					ok = false;
			if (((tmask[r] >> c) & 1u) && want[r][c] != v)
				ok = false;   // two terms of one class with different values
			tmask[r] |= 1u << c;
			want[r][c] = v;
		}
		if (!ok)
			continue;
		alive[r] = 1;
	}
	// A rule that can hold only when an earlier alive rule holds too (it
	// constrains every class the earlier one does, to the same values) is
	// never the first holding rule (match_pmr_cos scans in order): it is
	// dropped as unmatchable.  Repeated ACL lines and rules behind a broader
	// one then leave the candidate lists (nested-prefix ACLs fall to the
	// single-candidate engine).  Checked per distinct constrained-class set
	// of the earlier rules: O(rules x distinct sets).
	{
		std::map<uint32_t, std::set<std::vector<Key4>>> seen;   // class set -> value tuples
		for (uint32_t r = 0; r < nrules; ++r) {
			if (!alive[r])
				continue;
			for (auto &kv : seen) {
				const uint32_t m = kv.first;
				if ((m & ~tmask[r]) != 0u)
					continue;
				std::vector<Key4> t;
				for (uint32_t c = 0; c < ncls; ++c)
					if ((m >> c) & 1u)
						t.push_back(want[r][c]);
				if (kv.second.count(t)) {
					alive[r] = 0;
					break;
				}
			}
			if (!alive[r])
				continue;
			std::vector<Key4> t;
			for (uint32_t c = 0; c < ncls; ++c)
				if ((tmask[r] >> c) & 1u)
					t.push_back(want[r][c]);
			seen[tmask[r]].insert(t);
		}
	}
	for (uint32_t r = 0; r < nrules; ++r)
		if (alive[r])
			for (uint32_t c = 0; c < ncls; ++c)
				if ((tmask[r] >> c) & 1u)
					freq[c][want[r][c]]++;
	// primary class of every alive constrained rule: the class whose value
	// the fewest alive rules share (candidate engines file the rule under it)
	std::vector<uint32_t> prim_of(nrules, BV_NONE);
	std::vector<std::map<Key4, uint32_t>> filed(ncls);   // value -> #rules filed
	uint32_t max_list = 0, prim_mask = 0;
	for (uint32_t r = 0; r < nrules; ++r) {
		if (!alive[r] || tmask[r] == 0u)
			continue;
		uint32_t best = 0xFFFFFFFFu;
		for (uint32_t c = 0; c < ncls; ++c)
			if (((tmask[r] >> c) & 1u) && freq[c][want[r][c]] < best) {
				best = freq[c][want[r][c]];
				prim_of[r] = c;
			}
		const uint32_t c = prim_of[r];
		max_list = std::max(max_list, ++filed[c][want[r][c]]);
		prim_mask |= 1u << c;
	}
	// MI_CLS_NO_WIDE: candidate lists instead of wide rows; MI_CLS_NO_CAND1:
	// no single-candidate engine (A/B, tests)
	const bool wide_ok = !kn.no_wide, cand1_ok = !kn.no_cand1;
	const uint32_t mode = (ncls == 1 && !member) ? 0u
		: (nrules <= 32 ? 2u
		: ((cand1_ok && max_list <= 1u && nrules < 0xFFFFu) ? 4u
		: ((wide_ok && nrules <= 32 * BV_WIDE_WORDS) ? 3u : 1u)));
	std::vector<std::map<Key4, uint32_t>> kid(ncls);   // value -> key id (1..)
	for (uint32_t c = 0; c < ncls; ++c) {
		uint32_t id = 1;
		for (auto &kv : freq[c])
			kid[c][kv.first] = id++;
		if (id > 4096u)
			return bv_fail(kn, 2);
	}
	auto holds_class = [&](uint32_t r, uint32_t c, const Key4 *v) {
		return !((tmask[r] >> c) & 1u) || (v && want[r][c] == *v);
	};
	uint32_t wc_first = BV_NONE;   // first alive rule without a classified term
	for (uint32_t r = 0; r < nrules && wc_first == BV_NONE; ++r)
		if (alive[r] && tmask[r] == 0u)
			wc_first = r;
	// header (8) | classes (16 each) | results | [records] | per class: table [, lists].
	// Split class (direct blocks): the 16-word class record holds only what
	// the class is (kind, key words, masks, field descriptor); it is stored
	// once per distinct record in the hot region by assemble(), which
	// patches its index into the block's 6-word class info in header words
	// 2-7 (shared record, miss word, bucket count, table, m1, m2); the block
	// is header | table.  (Splitting the bitmap blocks' classes the same way
	// measured slower on config5: the per-lane rounds read more words.)
	const bool split = mode == 0u;
	blk.assign(mode == 0u ? 8u : 8u + BV_CLS_WORDS * ncls, 0);
	shared.clear();
	blk[0] = mode;
	blk[1] = ncls;
	blk[3] = wc_first;
	auto res_word = [&](uint32_t r) {
		return (rs[r].dst_cos & 0xffu) | (cs[rs[r].dst_cos].num_rules == 0 ? 0x100u : 0u) |
		       ((uint32_t)rs[r].mark << 16);
	};
	// direct blocks keep each rule's result word in the table slot itself
	// (no results array, no second lookup); the others index this array
	blk[2] = base + (uint32_t)blk.size();
	if (mode != 0u)
		for (uint32_t r = 0; r < nrules; ++r)
			blk.push_back(res_word(r));
	std::vector<std::vector<std::vector<uint32_t>>> lists(ncls);   // [class][key id] -> rules
	// wide rows: 8 words each (zero past the rule count), deduplicated.  Every
	// row id is assigned before the layout is emitted (mode 3 below): rows
	// are stored as two arrays of 4-word halves, so a row's value is the
	// hot-region word index of its first half and the second half is
	// blk[7] words further (16-B aligned; consecutive rows 16 B apart)
	const uint32_t nw = (nrules + 31u) / 32u;
	auto wide_row = [&](uint32_t c, const Key4 *v) {
		std::vector<uint32_t> w(BV_WIDE_WORDS, 0u);
		for (uint32_t r = 0; r < nrules; ++r)
			if (holds_class(r, c, v))
				w[r / 32u] |= 1u << (r % 32u);
		return w;
	};
	std::map<std::vector<uint32_t>, uint32_t> row_id;
	std::vector<const std::vector<uint32_t> *> rows;
	auto get_row = [&](const std::vector<uint32_t> &row) -> uint32_t {
		auto it = row_id.find(row);
		if (it != row_id.end())
			return it->second;
		const uint32_t id = (uint32_t)rows.size();
		auto ins = row_id.emplace(row, id).first;
		rows.push_back(&ins->first);
		return id;
	};
	std::vector<uint32_t> miss_id(ncls, 0);
	std::vector<std::vector<uint32_t>> key_row(ncls);
	uint32_t rows_at = 0;   // block-relative index of the first-halves array
	auto align4 = [&]() { while (blk.size() & 3u) blk.push_back(0); };
	if (mode == 2u) {
		uint32_t aw = 0;
		for (uint32_t r = 0; r < nrules; ++r)
			aw |= (uint32_t)alive[r] << r;
		blk[4] = aw;
	} else if (mode == 3u) {
		blk[6] = nw;
		blk[4] = (uint32_t)blk.size();   // the alive row, block-relative
		for (uint32_t i = 0; i < BV_WIDE_WORDS; ++i) {
			uint32_t aw = 0;
			for (uint32_t j = 0; j < 32u && 32u * i + j < nrules; ++j)
				aw |= (uint32_t)alive[32u * i + j] << j;
			blk.push_back(aw);
		}
		for (uint32_t c = 0; c < ncls; ++c) {
			miss_id[c] = get_row(wide_row(c, nullptr));
			for (auto &kv : kid[c])
				key_row[c].push_back(get_row(wide_row(c, &kv.first)));
		}
		align4();
		rows_at = (uint32_t)blk.size();
		const uint32_t R = (uint32_t)rows.size();
		blk[7] = 4u * R;
		for (uint32_t h = 0; h < 2; ++h)
			for (uint32_t j = 0; j < R; ++j)
				blk.insert(blk.end(), rows[j]->begin() + 4 * h, rows[j]->begin() + 4 * h + 4);
	} else if (mode == 4u) {
		// single-candidate records, 16-B aligned, RW = 1 + ncls rounded up
		// to 4 words: w0 = constrained-class mask (bit 31: never holds),
		// w[1 + c] = what class c must be: the masked value (one-word
		// classes) or the key id (longer keys).  Compact form (more than 3
		// classes, but no alive rule constrains more than 3): RW = 4, the
		// values of the constrained classes in class order (w[1 + j] for the
		// j-th set bit of the mask) -- a quarter to a half of the bytes, so
		// larger rule sets keep their hot region in LDS
		bool compact = ncls > 3u;
		for (uint32_t r = 0; r < nrules && compact; ++r)
			if (alive[r] && __builtin_popcount(tmask[r]) > 3)
				compact = false;
		const uint32_t RW = compact ? 4u : (1u + ncls + 3u) & ~3u;
		align4();
		blk[4] = base + (uint32_t)blk.size();
		blk[5] = RW;
		uint32_t lk = prim_mask;
		for (uint32_t c = 0; c < ncls; ++c)
			if (cls_list[c].nkey > 1u)
				lk |= 1u << c;   // key ids for the record compare
		blk[6] = lk;
		blk[7] = prim_mask;
		for (uint32_t r = 0; r < nrules; ++r) {
			std::vector<uint32_t> rec(RW, 0);
			if (alive[r]) {
				rec[0] = tmask[r];
				uint32_t j = 0;
				for (uint32_t c = 0; c < ncls; ++c)
					if ((tmask[r] >> c) & 1u)
						rec[1 + (compact ? j++ : c)] = cls_list[c].nkey == 1u
							? want[r][c][0] : kid[c][want[r][c]];
			} else {
				rec[0] = 0x80000000u;
			}
			blk.insert(blk.end(), rec.begin(), rec.end());
		}
	} else if (mode == 1u) {
		const uint32_t RW = 1u + (ncls + 1u) / 2u;
		blk[4] = base + (uint32_t)blk.size();
		blk[5] = RW;
		for (uint32_t c = 0; c < ncls; ++c)
			lists[c].resize(kid[c].size() + 1);
		for (uint32_t r = 0; r < nrules; ++r) {
			std::vector<uint32_t> rec(RW, 0);
			if (alive[r]) {
				rec[0] = tmask[r];
				uint32_t prim = BV_NONE, best = 0xFFFFFFFFu;
				for (uint32_t c = 0; c < ncls; ++c) {
					if (!((tmask[r] >> c) & 1u))
						continue;
					rec[1 + c / 2] |= kid[c][want[r][c]] << (16 * (c & 1u));
					const uint32_t f = freq[c][want[r][c]];
					if (f < best) {
						best = f;
						prim = c;
					}
				}
				if (prim != BV_NONE)
					lists[prim][kid[prim][want[r][prim]]].push_back(r);
			} else {
				rec[0] = 0x80000000u;   // never holds
			}
			blk.insert(blk.end(), rec.begin(), rec.end());
		}
	}
	auto first_live = [&](uint32_t c, const Key4 *v) -> uint32_t {
		for (uint32_t r = 0; r < nrules; ++r)
			if (alive[r] && holds_class(r, c, v))
				return r;
		return BV_NONE;
	};
	auto row_of = [&](uint32_t c, const Key4 *v) -> uint32_t {
		uint32_t w = 0;
		for (uint32_t r = 0; r < nrules; ++r)
			if (holds_class(r, c, v))
				w |= 1u << r;
		return w;
	};
	for (uint32_t c = 0; c < ncls; ++c) {
		const ClassKey &ck = cls_list[c];
		std::vector<Key4> keys;
		for (auto &kv : kid[c])
			keys.push_back(kv.first);
		uint32_t nb = 1, m1 = 1, m2 = 3;   // bucket count, multipliers
		std::vector<uint32_t> slot_of;
		// one-word keys: 2-slot buckets of 16 B; longer keys: 1 slot per bucket
		const uint32_t bsz = ck.nkey == 1 ? 2u : 1u;
		if (!cuckoo_place(keys, ck.nkey, bsz, nb, m1, m2, slot_of))
			return bv_fail(kn, 3);
		const uint32_t cbase = 8 + BV_CLS_WORDS * c;
		const uint32_t ib = mode == 0u ? 2u : 8u + 8u * c;   // split class info
		Rec16 rec;
		rec.fill(0u);
		auto setc = [&](uint32_t w, uint32_t v) {
			if (split)
				rec[w] = v;
			else
				blk[cbase + w] = v;
		};
		// slot: key words, value; one-word keys 2 words (two slots per 16-B
		// bucket), 2-3-word keys one 16-B slot, 4-word keys 32 B
		const uint32_t SW = bsz == 2u ? 2u : (ck.nkey <= 3u ? 4u : 8u);
		setc(0, ck.kind);
		setc(1, ck.nkey);
		const uint32_t fl0 = mode == 0u ? first_live(c, nullptr) : 0u;
		const uint32_t miss = mode == 0u ? (fl0 == BV_NONE ? 0u : res_word(fl0) | BV_RES_VALID)
			: (mode == 2u ? row_of(c, nullptr) : (mode == 3u ? base + rows_at + 4u * miss_id[c] : 0u));
		if (split)
			blk[ib + 1] = miss;
		else
			blk[cbase + 2] = miss;
		setc(3, ck.offset);
		setc(4, ck.size);
		for (int i = 0; i < 4; ++i)
			setc(5 + i, ck.mask[i]);
		if (split) {
			blk[ib + 2] = nb;
			blk[ib + 4] = m1;
			blk[ib + 5] = m2;
		} else {
			blk[cbase + 9] = nb;
			blk[cbase + 11] = m1;
			blk[cbase + 12] = m2;
		}
		{
			const bool special = ck.kind == MI_K_LEN || ck.kind == MI_K_PCP0 ||
					     ck.kind == MI_K_DSCP;
			const FDesc d = fdesc(ck.kind, ck.offset);
			if (d.add > 0xffffu || d.alt > 0xffffu)
				return bv_fail(kn, 4);   // custom offset past 64 KiB: linear scan
			// "always present" (custom frame) is F_L2, which every parsed
			// frame has
			const uint32_t gate = d.gate == ~0u ? F_L2 : d.gate;
			const uint32_t ac = d.altf == F_QINQ ? 1u
				: (d.altf == F_IPV4 ? 2u : (d.altf == F_AH ? 3u : 0u));
			const uint32_t fl = (special ? BVF_SPECIAL : 0u) |
				((ck.kind == MI_K_CUSTOM_FRAME || ck.kind == MI_K_CUSTOM_L3) ? BVF_CUSTOM : 0u) |
				(ck.kind == MI_K_CUSTOM_L3 ? BVF_L3 : 0u) | (ck.kind == K_L4PORT ? BVF_TAG : 0u);
			setc(BVC_AO, d.add | (d.alt << 16));
			setc(BVC_DESC, (gate & 0xffffffu) | (d.base << 24) | (ac << 26) | (fl << 28));
		}
		if (split)
			shared.emplace_back(ib, rec);
		align4();   // 16-B buckets / slots
		const uint32_t tbl_off = (uint32_t)blk.size();
		if (split)
			blk[ib + 3] = base + tbl_off;
		else
			blk[cbase + 10] = base + tbl_off;
		// empty slots keep key words 0 and value 0: a miss (every stored
		// value is non-zero)
		blk.resize(blk.size() + (size_t)nb * bsz * SW, 0);
		if (mode == 1u) {
			blk[cbase + 13] = base + (uint32_t)blk.size();
			for (auto &l : lists[c]) {
				if (l.size() > 255u)
					return bv_fail(kn, 5);   // degenerate: the linear scan is cheaper
				blk.insert(blk.end(), l.begin(), l.end());
			}
			if (blk.size() - (blk[cbase + 13] - base) > 4095u)
				return bv_fail(kn, 6);
		}
		for (uint32_t i = 0; i < keys.size(); ++i) {
			const uint32_t sl = tbl_off + slot_of[i] * SW;
			for (uint32_t j = 0; j < ck.nkey; ++j)
				blk[sl + j] = keys[i][j];
			uint32_t val;
			if (mode == 0u) {
				const uint32_t f = first_live(c, &keys[i]);
				val = f == BV_NONE ? BV_EMPTY : res_word(f) | BV_RES_VALID;
			} else if (mode == 2u) {
				val = row_of(c, &keys[i]);   // non-zero: the key's own rules
			} else if (mode == 3u) {
				val = base + rows_at + 4u * key_row[c][i];   // word index, non-zero
			} else if (mode == 4u) {
				// key id << 16 | 1 + the rule filed under this key (0: none)
				uint32_t cand = 0;
				for (uint32_t r = 0; r < nrules && !cand; ++r)
					if (prim_of[r] == c && want[r][c] == keys[i])
						cand = r + 1u;
				val = (kid[c][keys[i]] << 16) | cand;
			} else {
				const uint32_t id = kid[c][keys[i]];
				uint32_t off = 0;
				for (uint32_t q = 0; q < id; ++q)
					off += (uint32_t)lists[c][q].size();
				val = id | ((uint32_t)lists[c][id].size() << 12) | (off << 20);
			}
			blk[sl + ck.nkey] = val;
			if (bkv && (mode == 0u || mode == 2u)) {
				if (bkv->size() < ncls)
					bkv->resize(ncls);
				(*bkv)[c].emplace_back(keys[i], val);
			}
		}
	}
	return true;
}

// Rules of one CoS over more than BV_MAX_CLS key classes: split them into
// groups of at most BV_MAX_CLS classes (each rule into the first group its
// classes fit, in scan order) and build one block per group over the CoS's
// rule numbering, chained through header word 0 (mode | next << 8): the
// first holding rule is the smallest any block gives (bv_eval).  Appends
// the blocks to `hot`; returns the first block's index, 0 when the rules do
// not split into at most MAX_CHAIN groups (the linear scan is used).
#define MAX_CHAIN 4u
static uint32_t build_chain(const MiAsmKnobs &kn, const mi_cos_t *cs, const mi_rule_t *rs, const mi_term_t *ts,
			    uint32_t nrules, std::vector<uint32_t> &hot)
{
	std::vector<std::set<ClassKey>> groups;
	std::vector<std::vector<uint8_t>> member;
	for (uint32_t r = 0; r < nrules; ++r) {
		std::set<ClassKey> mine;
		for (uint32_t t = 0; t < rs[r].num_terms; ++t) {
			ClassKey ck;
			if (class_of(kn, ts[rs[r].term_begin + t], ck))
				mine.insert(ck);
		}
		size_t g = 0;
		for (; g < groups.size(); ++g) {
			std::set<ClassKey> u = groups[g];
			u.insert(mine.begin(), mine.end());
			if (u.size() <= BV_MAX_CLS) {
				groups[g].swap(u);
				break;
			}
		}
		if (g == groups.size()) {
			if (groups.size() == MAX_CHAIN || mine.size() > BV_MAX_CLS) {
				if (kn.verbose)
					fprintf(stderr, "mi_cls: rules do not split into %u blocks\n", MAX_CHAIN);
				return 0;
			}
			groups.push_back(mine);
			member.emplace_back(nrules, 0);
		}
		member[g][r] = 1;
	}
	if (groups.size() < 2)
		return 0;
	std::vector<std::vector<uint32_t>> blks(groups.size());
	std::vector<uint32_t> at(groups.size());
	size_t pos = hot.size();
	for (size_t g = 0; g < groups.size(); ++g) {
		pos = (pos + 3u) & ~(size_t)3u;   // blocks start 16-B aligned
		at[g] = (uint32_t)pos;
		SharedRecs shared;
		if (!build_bv(kn, cs, rs, ts, nrules, at[g], blks[g], shared, &member[g]) ||
		    !shared.empty() || (blks[g][0] & ~0xffu)) {
			if (kn.verbose)
				fprintf(stderr, "mi_cls: chain block %zu of %zu not built\n", g, groups.size());
			return 0;
		}
		pos += blks[g].size();
	}
	if (pos >= (1u << 24))
		return 0;
	for (size_t g = 0; g < groups.size(); ++g) {
		if (g + 1 < groups.size())
			blks[g][0] |= at[g + 1] << 8;
		while (hot.size() < at[g])
			hot.push_back(0);
		hot.insert(hot.end(), blks[g].begin(), blks[g].end());
	}
	return at[0];
}

// The program runs the tree kernels (DIV): a rule whose destination has
// rules, or an error CoS with rules next to a default CoS with rules -- lanes
// of a wave may then sit on different CoS with rules in one round.
// MI_CLS_DIV=0|1 forces the choice (A/B runs).
static bool program_is_tree(const MiAsmKnobs &kn, const Tbl &t)
{
	if (kn.div >= 0)
		return kn.div != 0;
	for (uint32_t r = 0; r < t.h->num_rules; ++r)
		if (t.cs[t.rs[r].dst_cos].num_rules != 0)
			return true;
	return t.h->error_cos >= 0 && t.h->default_cos >= 0 && t.cs[t.h->error_cos].num_rules &&
	       t.cs[t.h->default_cos].num_rules;
}

// ---- assembly of the hot region ----
// Joint tables (tree programs): CoS whose blocks have the same shape --
// direct blocks sharing a class record, bitmap blocks over the same class
// records (a tree level of CoS keyed on the same fields) -- get one cuckoo
// table per class over (key, CoS) instead of a table each.  A round whose
// pending lanes all sit on CoS of one such group evaluates them with the
// group's words in SGPRs (no per-lane block or class-record reads); the
// per-lane rounds probe the same tables.
struct JClass {
	Rec16 rec;
	uint32_t flags, nkj, nb, m1, m2;
	std::vector<Key4> keys;
	std::vector<uint32_t> vals, slot_of;
};
struct Joint {
	uint32_t kind;
	std::vector<uint32_t> members;
	std::vector<JClass> cls;
};

// The hot region under construction (offsets relative to its start): the
// CoS table, then the blocks, the joint groups and the shared class records
struct Hot {
	std::vector<uint32_t> w;
	std::vector<Joint> joints;
	std::vector<uint32_t> gid_of;                  // per CoS: 1 + its joint group (0: none)
	std::vector<std::vector<uint32_t>> blk0;       // per member CoS: its block, built at offset 0
	std::vector<Rec16> drec;                       // per direct member CoS: its class record
	// direct blocks' class records, one copy per distinct record -> patch words
	std::map<Rec16, std::vector<uint32_t>> shared_users;
	// per joint group and class: member words to point at its table
	// (direct: header word 4; bitmap: class record word 9)
	std::vector<std::vector<std::vector<uint32_t>>> joint_patch;
	void align4()   // blocks, rows, buckets start 16-B aligned
	{
		while (w.size() & 3u)
			w.push_back(0);
	}
};

// Shape of a block that may join a group (empty: it may not): a direct
// block's shared class record, or a bitmap block's class records without
// the words that are the CoS's own.
static std::vector<uint32_t> joint_shape(const std::vector<uint32_t> &blk, const SharedRecs &shared,
					 const BlockKV &bkv, Rec16 &drec)
{
	std::vector<uint32_t> shape;
	if (blk[0] == 0u && shared.size() == 1 && shared[0].second[1] <= 3u && bkv.size() == 1) {
		drec = shared[0].second;
		shape.assign(shared[0].second.begin(), shared[0].second.end());
		shape.insert(shape.begin(), 0u);
	} else if (blk[0] == 2u && bkv.size() == blk[1]) {
		shape.push_back(2u);
		shape.push_back(blk[1]);
		for (uint32_t c = 0; c < blk[1]; ++c) {
			Rec16 r;
			for (uint32_t i = 0; i < 16; ++i)
				r[i] = blk[8u + 16u * c + i];
			r[2] = r[9] = r[10] = r[11] = r[12] = r[13] = 0u;   // the CoS's own
			if (r[1] > 3u)
				return {};
			shape.insert(shape.end(), r.begin(), r.end());
		}
	}
	return shape;
}

// Joint-group planning: every block's keys and values (built at relative
// offsets, only the values are used), the CoS grouped by shape, and one
// table per class of every group of two or more.
static void plan_joints(const MiAsmKnobs &kn, const Tbl &t, Hot &H)
{
	const uint32_t num_cos = t.h->num_cos;
	std::vector<BlockKV> bkv(num_cos);
	std::map<std::vector<uint32_t>, std::vector<uint32_t>> groups;   // shape -> CoS
	for (uint32_t s = 0; s < num_cos; ++s) {
		if (!t.cs[s].valid || t.cs[s].num_rules == 0)
			continue;
		std::vector<uint32_t> blk;
		SharedRecs shared;
		if (!build_bv(kn, t.cs, t.rs + t.cs[s].rule_begin, t.ts, t.cs[s].num_rules, 0, blk, shared,
			      nullptr, &bkv[s]))
			continue;
		const std::vector<uint32_t> shape = joint_shape(blk, shared, bkv[s], H.drec[s]);
		if (shape.empty())
			continue;
		H.blk0[s].swap(blk);
		groups[shape].push_back(s);
	}
	for (auto &g : groups) {
		if (g.second.size() < 2 || H.joints.size() == 127)
			continue;
		Joint j;
		j.kind = g.first[0];
		j.members = g.second;
		const uint32_t ncls = j.kind == 0u ? 1u : g.first[1];
		bool ok = true;
		for (uint32_t c = 0; c < ncls && ok; ++c) {
			JClass jc;
			const uint32_t at = j.kind == 0u ? 1u : 2u + 16u * c;
			std::copy(g.first.begin() + at, g.first.begin() + at + 16, jc.rec.begin());
			const uint32_t nk = jc.rec[1];
			// one-word keys with 8 bits no rule can set (outside the mask
			// and the merged ports' protocol tag at bit rec[3]) take the
			// CoS slot there; longer keys get it appended
			const uint32_t used = jc.rec[5] | ((jc.rec[BVC_DESC] >> 28) & BVF_TAG
							   ? 3u << jc.rec[3] : 0u);
			uint32_t sh = 0;
			while (sh <= 24u && ((used >> sh) & 0xFFu))
				++sh;
			const bool one = nk == 1u && sh <= 24u && num_cos <= 256u;
			if (!one && nk >= 4u) {   // no room for the CoS word
				ok = false;
				break;
			}
			jc.flags = one ? (BVJ_ONEWORD | (sh << BVJ_SHIFT)) : BVJ_APPEND;
			jc.nkj = one ? 1u : nk + 1u;
			for (uint32_t s : j.members)
				for (auto &kv : bkv[s][c]) {
					Key4 k = kv.first;
					if (one)
						k[0] |= s << sh;
					else
						k[nk] = s;
					jc.keys.push_back(k);
					jc.vals.push_back(kv.second);
				}
			ok = cuckoo_place(jc.keys, jc.nkj, jc.nkj == 1u ? 2u : 1u, jc.nb, jc.m1, jc.m2,
					  jc.slot_of);
			j.cls.push_back(std::move(jc));
		}
		if (!ok)
			continue;
		H.joints.push_back(std::move(j));
		for (uint32_t s : H.joints.back().members)
			H.gid_of[s] = (uint32_t)H.joints.size();
	}
}

// Per-CoS blocks: a joint group's member gets its header (direct), or
// header, class records and results (bitmap) -- its tables are the group's
// (emit_joints patches them in); every other CoS its own block, or (flat
// programs: the DIV kernels evaluate no chains, mi_cls_dev.h bv_eval) a
// chain of blocks when it has more key classes than a block holds.
static void emit_cos_blocks(const MiAsmKnobs &kn, const Tbl &t, bool tree, Hot &H)
{
	std::vector<uint32_t> &hot = H.w;
	for (uint32_t s = 0; s < t.h->num_cos; ++s) {
		const mi_cos_t &cos = t.cs[s];
		if (!cos.valid || cos.num_rules == 0)
			continue;
		H.align4();
		const uint32_t base = (uint32_t)hot.size();
		if (H.gid_of[s]) {
			const uint32_t g = H.gid_of[s] - 1;
			const Joint &j = H.joints[g];
			const std::vector<uint32_t> &b0 = H.blk0[s];
			std::vector<uint32_t> hd;
			if (j.kind == 0u) {
				hd.assign(b0.begin(), b0.begin() + 8);
				hd[1] |= j.cls[0].flags;
				H.shared_users[H.drec[s]].push_back(base + 2u);
				H.joint_patch[g][0].push_back(base + 4u);
			} else {
				const uint32_t ncls = b0[1], rec_end = 8u + 16u * ncls;
				hd.assign(b0.begin(), b0.begin() + rec_end + cos.num_rules);
				hd[2] = base + rec_end;   // the results array follows the records
				for (uint32_t c = 0; c < ncls; ++c) {
					hd[8u + 16u * c + 13u] = j.cls[c].flags;
					H.joint_patch[g][c].push_back(base + 8u + 16u * c + 9u);
				}
			}
			hot[COS_WORDS * s + C_BV] = base | (H.gid_of[s] << 24);
			hot.insert(hot.end(), hd.begin(), hd.end());
			continue;
		}
		std::vector<uint32_t> blk;
		SharedRecs shared;
		if (build_bv(kn, t.cs, t.rs + cos.rule_begin, t.ts, cos.num_rules, base, blk, shared)) {
			hot[COS_WORDS * s + C_BV] = base;
			hot.insert(hot.end(), blk.begin(), blk.end());
			for (auto &sh : shared)
				H.shared_users[sh.second].push_back(base + sh.first);
		} else if (!tree) {
			const uint32_t first = build_chain(kn, t.cs, t.rs + cos.rule_begin, t.ts, cos.num_rules, hot);
			if (first)
				hot[COS_WORDS * s + C_BV] = first | 0x80000000u;
		}
	}
}

// The joint groups: per class a table, miss values per CoS slot and (bitmap)
// its class record; per group alive rows and results offsets per CoS slot;
// an 8-word header + 8 words per class, found through a directory of group
// offsets.  Returns the directory's word (DH_JOINT; 0: no groups).
// The per-CoS-slot arrays span the group's slots only (a tree level's CoS
// are usually consecutive): their words are stored as (array start - lowest
// member slot), indexed by the slot itself (the CoS entries precede every
// array, so this never wraps).
static uint32_t emit_joints(const MiAsmKnobs &kn, Hot &H)
{
	std::vector<uint32_t> &hot = H.w;
	std::vector<uint32_t> dir;
	for (size_t g = 0; g < H.joints.size(); ++g) {
		const Joint &j = H.joints[g];
		const uint32_t lo = *std::min_element(j.members.begin(), j.members.end());
		const uint32_t span = *std::max_element(j.members.begin(), j.members.end()) - lo + 1u;
		std::vector<uint32_t> info(8u + 8u * j.cls.size(), 0u);
		info[0] = j.kind;
		info[1] = (uint32_t)j.cls.size();
		if (j.kind == 2u) {
			const uint32_t alive = (uint32_t)hot.size() - lo;
			hot.resize(hot.size() + 2u * span, 0);
			for (uint32_t x : j.members) {
				const uint32_t b = hot[COS_WORDS * x + C_BV] & C_BV_OFF;
				hot[alive + x] = H.blk0[x][4];
				hot[alive + span + x] = hot[b + 2];   // its results array
			}
			info[2] = alive;
			info[3] = alive + span;
		}
		for (size_t c = 0; c < j.cls.size(); ++c) {
			const JClass &jc = j.cls[c];
			const uint32_t bsz = jc.nkj == 1u ? 2u : 1u;
			const uint32_t SW = bsz == 2u ? 2u : (jc.nkj <= 3u ? 4u : 8u);
			H.align4();
			const uint32_t tbl = (uint32_t)hot.size();
			hot.resize(hot.size() + (size_t)jc.nb * bsz * SW, 0);
			for (size_t i = 0; i < jc.keys.size(); ++i) {
				const uint32_t sl = tbl + jc.slot_of[i] * SW;
				for (uint32_t q = 0; q < jc.nkj; ++q)
					hot[sl + q] = jc.keys[i][q];
				hot[sl + jc.nkj] = jc.vals[i];
			}
			const uint32_t miss = (uint32_t)hot.size() - lo;
			hot.resize(hot.size() + span, 0);
			for (uint32_t x : j.members)
				hot[miss + x] = j.kind == 0u ? H.blk0[x][3] : H.blk0[x][8u + 16u * c + 2u];
			for (uint32_t w : H.joint_patch[g][c]) {   // nb, table, m1, m2
				hot[w] = jc.nb;
				hot[w + 1] = tbl;
				hot[w + 2] = jc.m1;
				hot[w + 3] = jc.m2;
			}
			uint32_t *ci = &info[8u + 8u * c];
			ci[1] = jc.nb;
			ci[2] = tbl;
			ci[3] = jc.m1;
			ci[4] = jc.m2;
			ci[5] = miss;
			ci[6] = jc.flags;
			if (j.kind == 2u) {   // the class record, read with scalar loads
				H.align4();
				ci[0] = (uint32_t)hot.size();
				hot.insert(hot.end(), jc.rec.begin(), jc.rec.end());
			}
		}
		H.align4();
		const uint32_t at = (uint32_t)hot.size();
		dir.push_back(at);
		hot.insert(hot.end(), info.begin(), info.end());
		if (j.kind == 0u)   // class 0's record word: the shared record
			H.shared_users[j.cls[0].rec].push_back(at + 8u);
	}
	if (H.joints.empty())
		return 0;
	H.align4();
	const uint32_t joint_info = (uint32_t)hot.size();
	hot.insert(hot.end(), dir.begin(), dir.end());
	if (kn.verbose) {
		fprintf(stderr, "mi_cls: %zu joint groups\n", H.joints.size());
		for (auto &j : H.joints)
			for (auto &jc : j.cls)
				fprintf(stderr, "mi_cls:  kind %u members %zu keys %zu key words %u buckets %u\n",
					j.kind, j.members.size(), jc.keys.size(), jc.nkj, jc.nb);
	}
	return joint_info;
}

// Furthest bytes the terms (and the hash-queue tuple) read, per base: the
// kernel's window predictor only, correctness never depends on these.
static void window_ends(const Tbl &t, uint32_t *w)
{
	uint32_t end[3] = { 0, 0, 0 };
	for (uint32_t i = 0; i < t.h->num_terms; ++i) {
		const mi_term_t &tm = t.ts[i];
		uint32_t base = FB_FRAME, e = 0;
		switch (tm.kind) {
		case MI_K_LEN: case MI_K_NEVER: case MI_K_ALWAYS:
			break;
		case MI_K_PCP0: e = 16; break;
		case MI_K_DSCP: base = FB_L3; e = 4; break;
		case MI_K_CUSTOM_FRAME: e = tm.offset + tm.size + 4u; break;
		case MI_K_CUSTOM_L3: base = FB_L3; e = tm.offset + tm.size + 4u; break;
		default: {
			const FDesc d = fdesc(tm.kind, 0);
			base = d.base;
			e = std::max(d.add, d.alt) + 4u * kind_words(tm.kind, tm.size);
		}
		}
		end[base] = std::max(end[base], std::min(e, 0xFFFFu));
	}
	for (uint32_t s = 0; s < t.h->num_cos; ++s)
		if (t.cs[s].num_queue > 1) {   // Toeplitz tuple (rss_hash)
			end[FB_L3] = std::max(end[FB_L3], 40u);
			end[FB_L4] = std::max(end[FB_L4], 4u);
		}
	w[DH_FREND] = end[FB_FRAME];
	w[DH_L3END] = end[FB_L3];
	w[DH_L4END] = end[FB_L4];
}

// Cold region: the 16-word rule records at prog_off (already zeroed in w),
// the terms that do not fit them appended after the last record.
static int emit_rules(const Tbl &t, size_t prog_off, std::vector<uint32_t> &w)
{
	std::vector<uint32_t> ext;
	const size_t ext_base = (size_t)t.h->num_rules * REC_WORDS;
	for (uint32_t r = 0; r < t.h->num_rules; ++r) {
		const mi_rule_t &rule = t.rs[r];
		uint32_t *rec = &w[prog_off + (size_t)r * REC_WORDS];
		uint32_t used = 2, n_in = 0, n_ext = 0;
		size_t ext_begin = ext_base + ext.size();
		for (uint32_t i = 0; i < rule.num_terms; ++i) {
			uint32_t tw[12];
			uint32_t n = encode_term(t.ts[rule.term_begin + i], tw);
			if (n_ext == 0 && used + n <= REC_WORDS) {
				memcpy(rec + used, tw, n * sizeof(uint32_t));
				used += n;
				n_in++;
			} else {
				ext.insert(ext.end(), tw, tw + n);
				n_ext++;
			}
		}
		if (ext_begin >= (1u << 24))
			return -E2BIG;
		rec[0] = n_in | (n_ext << 8) | ((uint32_t)rule.mark << 16);
		rec[1] = rule.dst_cos | ((uint32_t)(n_ext ? ext_begin : 0) << 8);
	}
	w.insert(w.end(), ext.begin(), ext.end());
	return 0;
}

// Assemble the (validated) mi_cls.h table into the device encoding.
static int assemble(const MiAsmKnobs &kn, const Tbl &t, bool tree, std::vector<uint32_t> &w)
{
	const mi_tbl_hdr_t *h = t.h;
	// hot region: CoS table then the BV blocks (offsets relative to hot_off)
	Hot H;
	H.w.assign((size_t)COS_WORDS * h->num_cos, 0);
	for (uint32_t s = 0; s < h->num_cos; ++s) {
		uint32_t *c = &H.w[COS_WORDS * s];
		c[C_NR] = t.cs[s].num_rules;
		c[C_META] = (uint32_t)t.cs[s].action | ((uint32_t)t.cs[s].num_queue << 8) |
			    ((uint32_t)t.cs[s].hash_proto << 16) | ((uint32_t)t.cs[s].index << 24);
		c[C_REC0] = t.cs[s].rule_begin;
	}
	H.gid_of.assign(h->num_cos, 0);
	H.blk0.resize(h->num_cos);
	H.drec.resize(h->num_cos);
	uint32_t joint_info = 0;   // hot-region word of the joint groups' directory
	if (!kn.no_bv) {
		if (tree && !kn.no_joint)
			plan_joints(kn, t, H);
		H.joint_patch.resize(H.joints.size());
		for (size_t g = 0; g < H.joints.size(); ++g)
			H.joint_patch[g].resize(H.joints[g].cls.size());
		emit_cos_blocks(kn, t, tree, H);
		joint_info = emit_joints(kn, H);
		for (auto &kv : H.shared_users) {   // the shared class records
			H.align4();
			const uint32_t at = (uint32_t)H.w.size();
			H.w.insert(H.w.end(), kv.first.begin(), kv.first.end());
			for (uint32_t p : kv.second)
				H.w[p] = at;
		}
	}
	const std::vector<uint32_t> &hot = H.w;
	const uint32_t hot_off = DH_WORDS;
	const size_t prog_off = hot_off + hot.size();
	w.assign(prog_off + (size_t)h->num_rules * REC_WORDS, 0);
	std::copy(hot.begin(), hot.end(), w.begin() + hot_off);
	w[DH_MAGIC] = DEV_MAGIC;
	w[DH_NCOS] = h->num_cos;
	w[DH_DEFAULT] = (uint32_t)h->default_cos;
	w[DH_ERROR] = (uint32_t)h->error_cos;
	w[DH_DEFAULT_VALID] = h->default_valid;
	w[DH_USED] = h->used_kinds;
	w[DH_MAX_HOPS] = h->max_hops;
	w[DH_HOT_OFF] = hot_off;
	w[DH_HOT_WORDS] = (uint32_t)hot.size();
	w[DH_PROG_OFF] = (uint32_t)prog_off;
	w[DH_JOINT] = joint_info;
	window_ends(t, w.data());
	const int rc = emit_rules(t, prog_off, w);
	if (rc)
		return rc;
	w.resize(w.size() + 16, 0);
	w[DH_TOTAL] = (uint32_t)w.size();
	return 0;
}

// The default CoS's classification block, if the program has one (0: none).
static uint32_t default_block(const uint32_t *w)
{
	const int32_t d = (int32_t)w[DH_DEFAULT];
	if (d < 0 || !w[DH_DEFAULT_VALID])
		return 0u;
	const uint32_t *hot = w + w[DH_HOT_OFF];
	return hot[COS_WORDS * (uint32_t)d + C_NR] ? hot[COS_WORDS * (uint32_t)d + C_BV] & C_BV_OFF
						 : 0u;
}

// Source text of the compile-time block a program-specialised flat kernel
// uses (DescC in mi_cls_dev.h): the default CoS's classification block words
// (header, then 16 words per class record for modes 1-4; zero-padded by 16
// words) and, for a direct block, its shared class record.
static std::string spec_source_chain(const uint32_t *hot, uint32_t bv);

static std::string spec_source(const uint32_t *hot, uint32_t bv, int fm)
{
	if (fm == FM_CHAIN)
		return spec_source_chain(hot, bv);
	const uint32_t *b = hot + bv;
	const uint32_t mode = b[0] & 0xffu;   // | next block of a chain << 8
	// header and class records; a wide bitmap block also reads its alive
	// row block-relative (bv_eval: blk(ar + i))
	uint32_t nw = mode == 0u ? 8u : 8u + BV_CLS_WORDS * b[1];
	if (mode == 3u)
		nw = std::max(nw, b[4] + BV_WIDE_WORDS);
	std::string s = "struct MiSpec {\n\tstatic constexpr uint32_t blk[] = {";
	char t[32];
	for (uint32_t i = 0; i < nw + 16u; ++i) {
		snprintf(t, sizeof(t), "%s0x%xu", i ? "," : "", i < nw ? b[i] : 0u);
		s += t;
	}
	s += "};\n\tstatic constexpr uint32_t root[16] = {";
	for (uint32_t i = 0; i < 16u; ++i) {
		snprintf(t, sizeof(t), "%s0x%xu", i ? "," : "", mode == 0u ? hot[b[2] + i] : 0u);
		s += t;
	}
	snprintf(t, sizeof(t), "%d", fm);
	s += "};\n};\n#define MI_SPEC_FM ";
	s += t;
	s += "\n";
	return s;
}

// The default CoS's block word when one round on it decides every packet
// (a valid default CoS with rules, all of which lead to CoS without rules),
// else 0.  MI_CLS_NO_FLAT disables the flat kernels (A/B, tests).
static uint32_t one_round_block(const MiAsmKnobs &kn, const Tbl &t, const uint32_t *w)
{
	const int32_t d = t.h->default_cos;
	if (d < 0 || !t.h->default_valid || !t.cs[d].num_rules || kn.no_flat)
		return 0;
	bool leaves = true;
	for (uint32_t r = 0; r < t.cs[d].num_rules && leaves; ++r)
		leaves = t.cs[t.rs[t.cs[d].rule_begin + r].dst_cos].num_rules == 0;
	return leaves ? w[w[DH_HOT_OFF] + COS_WORDS * (uint32_t)d + C_BV] & (C_BV_OFF | 0x80000000u) : 0u;
}

// Source text of a chain's compile-time blocks (FM_CHAIN): every block's
// words (header, class records, a wide bitmap's alive row) one after the
// other, their offsets and engines.
static std::string spec_source_chain(const uint32_t *hot, uint32_t bv)
{
	std::vector<uint32_t> words, offs, modes;
	for (uint32_t o = bv & 0x7fffffffu; o;) {
		const uint32_t *b = hot + o;
		const uint32_t mode = b[0] & 0xffu;
		uint32_t nw = 8u + BV_CLS_WORDS * b[1];
		if (mode == 3u)
			nw = std::max(nw, b[4] + BV_WIDE_WORDS);
		offs.push_back((uint32_t)words.size());
		modes.push_back(mode);
		words.insert(words.end(), b, b + nw);
		while (words.size() & 3u)
			words.push_back(0u);
		o = b[0] >> 8;
	}
	words.insert(words.end(), 16, 0u);
	std::string s = "struct MiSpec {\n\tstatic constexpr uint32_t blk[] = {";
	char t[32];
	for (size_t i = 0; i < words.size(); ++i) {
		snprintf(t, sizeof(t), "%s0x%xu", i ? "," : "", words[i]);
		s += t;
	}
	s += "};\n\tstatic constexpr uint32_t root[16] = {0u};\n\tstatic constexpr uint32_t nblk = ";
	s += std::to_string(offs.size());
	s += ";\n\tstatic constexpr uint32_t boff[] = {";
	for (size_t i = 0; i < offs.size(); ++i)
		s += (i ? "," : "") + std::to_string(offs[i]) + "u";
	s += "};\n\tstatic constexpr uint32_t bmode[] = {";
	for (size_t i = 0; i < modes.size(); ++i)
		s += (i ? "," : "") + std::to_string(modes[i]) + "u";
	s += "};\n};\n#define MI_SPEC_FM " + std::to_string(FM_CHAIN) + "\n";
	return s;
}

// The plan of a CoS tree (tree-plan kernels, mi_cls_dev.h plan_eval): the
// joint groups of the tree's levels below the default CoS, when they cover
// it -- every rule of the default CoS leads to a leaf or to a CoS of group
// g1, every rule of those CoS to a leaf or to a CoS of g2, and so on, the
// last level's rules all to leaves.  Returns the group ids (1-based, as in
// the CoS entries' C_BV bits 24-30) per round after the first; empty: no
// plan (the program keeps the generic tree kernel).  MI_CLS_NO_PLAN=1
// disables them (A/B, tests).
#define PLAN_MAX 4u
static std::vector<uint32_t> tree_plan(const MiAsmKnobs &kn, const Tbl &t, bool tree, const uint32_t *w)
{
	const mi_cos_t *tc = t.cs;
	const uint32_t *hot = w + w[DH_HOT_OFF];
	std::vector<uint32_t> plan;
	if (kn.no_plan || !tree || !default_block(w) || !w[DH_JOINT])
		return plan;
	std::set<uint32_t> level = { (uint32_t)t.h->default_cos };
	for (uint32_t depth = 0; depth <= PLAN_MAX; ++depth) {
		std::set<uint32_t> next;
		for (uint32_t s : level)
			for (uint32_t r = 0; r < tc[s].num_rules; ++r) {
				const uint32_t d = t.rs[tc[s].rule_begin + r].dst_cos;
				if (tc[d].num_rules)
					next.insert(d);
			}
		if (next.empty())
			return plan;   // the last level leads to leaves only: covered
		if (depth == PLAN_MAX)
			break;
		const uint32_t g = (hot[COS_WORDS * *next.begin() + C_BV] >> 24) & 0x7fu;
		for (uint32_t d : next)
			if (g == 0u || ((hot[COS_WORDS * d + C_BV] >> 24) & 0x7fu) != g)
				return {};
		plan.push_back(g);
		level.swap(next);
	}
	return {};
}

// Source text of a tree plan (appended to the default block's MiSpec): per
// round the group id, its info words (group header + 8 words per class, as
// in the hot region) and its class records.
static std::string spec_source_plan(const uint32_t *w, const std::vector<uint32_t> &plan)
{
	const uint32_t *hot = w + w[DH_HOT_OFF];
	const uint32_t *dir = hot + w[DH_JOINT];
	std::string gid, info, rec;
	char t[32];
	for (size_t i = 0; i < plan.size(); ++i) {
		const uint32_t *ji = hot + dir[plan[i] - 1u];
		const uint32_t ncls = ji[0] == 0u ? 1u : ji[1];
		gid += (i ? "," : "") + std::to_string(plan[i]) + "u";
		info += i ? ",{" : "{";
		rec += i ? ",{" : "{";
		for (uint32_t k = 0; k < 8u + 8u * BV_MAX_CLS; ++k) {
			snprintf(t, sizeof(t), "%s0x%xu", k ? "," : "", k < 8u + 8u * ncls ? ji[k] : 0u);
			info += t;
		}
		for (uint32_t c = 0; c < BV_MAX_CLS; ++c) {
			rec += c ? ",{" : "{";
			for (uint32_t k = 0; k < 16u; ++k) {
				snprintf(t, sizeof(t), "%s0x%xu", k ? "," : "", c < ncls ? hot[ji[8u + 8u * c] + k] : 0u);
				rec += t;
			}
			rec += "}";
		}
		info += "}";
		rec += "}";
	}
	const std::string n = std::to_string(plan.size());
	return "\tstatic constexpr uint32_t nplan = " + n + ";\n\tstatic constexpr uint32_t gid[" + n +
	       "] = {" + gid + "};\n\tstatic constexpr uint32_t ginfo[" + n + "][" +
	       std::to_string(8u + 8u * BV_MAX_CLS) + "] = {" + info +
	       "};\n\tstatic constexpr uint32_t grec[" + n + "][" + std::to_string(BV_MAX_CLS) + "][16] = {" +
	       rec + "};\n";
}

std::string mi_asm_spec_program(const MiProgram &p, int nw, bool lt, bool ck, std::string &inst)
{
	// flat engine fm, or -1: the general kernel with per-lane tree rounds
	// and the plan's rounds compiled in
	const uint32_t *w = p.w.data();
	const int fm = p.spec_mode;
	char t[96];
	snprintf(t, sizeof(t), "mi_cls_kernel<%s, %s, %d, %d, %s, MiSpec>", lt ? "true" : "false",
		 fm < 0 ? "true" : "false", nw, fm, ck ? "true" : "false");
	inst = t;
	std::string spec = spec_source(w + w[DH_HOT_OFF], default_block(w), fm);
	if (!p.plan.empty()) {   // a tree plan: its rounds go into the struct
		const size_t at = spec.find("};\n#define MI_SPEC_FM");
		spec.insert(at, spec_source_plan(w, p.plan));
	}
	return "#include \"mi_cls_dev.h\"\n" + spec + "template __global__ void " + inst + "(KArgs);\n";
}

int mi_asm_compile(const void *tbl, size_t bytes, const MiAsmKnobs &kn, MiProgram &out)
{
	int rc = validate_tbl(tbl, bytes);
	if (rc)
		return rc;
	const Tbl t(tbl);
	out = MiProgram();
	out.tree = program_is_tree(kn, t);
	rc = assemble(kn, t, out.tree, out.w);
	if (rc)
		return rc;
	const uint32_t *w = out.w.data();
	out.hot_words = w[DH_HOT_WORDS];
	// the flat engine: none without a one-round block, or with a chain of
	// blocks (specialised kernels only; so are candidate lists, mode 1).
	// A specialised kernel compiles in the flat engine, or FM_CHAIN (the
	// chain's blocks and their engines become compile-time constants too)
	const uint32_t bv = one_round_block(kn, t, w);
	out.flat_mode = (!bv || (bv >> 31)) ? -1 : (int)w[w[DH_HOT_OFF] + bv];
	out.spec_mode = (bv >> 31) ? FM_CHAIN : out.flat_mode;
	out.plan = tree_plan(kn, t, out.tree, w);
	return 0;
}
