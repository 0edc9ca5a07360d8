// asm_check -- stand-alone driver of the rule-program assembler
// (odp_amd/csrc/mi_cls_asm.cpp), built with -fsanitize=address,undefined by
// tests/test_asm_check.py and run as a child process.
//
//   asm_check [--hostile] BLOB...
//
// Per table blob (odp_amd_cls_compile output) and knob set: assemble, probe
// every key of every cuckoo table of the program again with the shared
// bv_fold / bv_bucket, build the specialised kernel's source text where the
// program has one, and print one line of facts.  --hostile: the first blob
// is also fed truncated and corrupted; every such table must be -EINVAL.
// Exit status 0 when every check held.
#include "mi_cls_asm.h"

#include "mi_cls.h"
#include "mi_cls_prog.h"

#include <errno.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <set>

static int g_bad;

#define CHECK(x, ...)                                                          \
	do {                                                                   \
		if (!(x)) {                                                    \
			fprintf(stderr, "asm_check: " __VA_ARGS__);            \
			fprintf(stderr, " [%s]\n", #x);                        \
			++g_bad;                                               \
		}                                                              \
	} while (0)

static uint64_t fnv1a(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull)
{
	const uint8_t *b = (const uint8_t *)p;
	for (size_t i = 0; i < n; ++i)
		h = (h ^ b[i]) * 0x100000001b3ull;
	return h;
}

// One cuckoo table: nk key words per slot, then the value (0: empty slot)
struct Probe {
	const MiProgram &p;
	std::set<uint32_t> seen;   // tables probed (joint tables have many users)
	size_t tables = 0, keys = 0;

	void table(uint32_t nk, uint32_t nb, uint32_t tbl, uint32_t m1, uint32_t m2)
	{
		if (!seen.insert(tbl).second)
			return;
		const uint32_t *hot = p.w.data() + p.w[DH_HOT_OFF];
		const uint32_t bsz = nk == 1u ? 2u : 1u, SW = bsz == 2u ? 2u : (nk <= 3u ? 4u : 8u);
		CHECK(nk >= 1 && nk <= 4 && nb >= 1 && nb <= 65536u, "table %u: nk %u nb %u", tbl, nk, nb);
		CHECK((tbl & 3u) == 0 && (uint64_t)tbl + (uint64_t)nb * bsz * SW <= p.hot_words,
		      "table %u: %u buckets past the hot region (%u words)", tbl, nb, p.hot_words);
		if (g_bad)
			return;
		++tables;
		for (uint32_t s = 0; s < nb * bsz; ++s) {
			const uint32_t *sl = hot + tbl + s * SW;
			if (sl[nk] == 0u)
				continue;
			uint32_t k[4] = { 0, 0, 0, 0 };
			memcpy(k, sl, nk * sizeof(uint32_t));
			const uint32_t x = nk == 1u ? k[0] : bv_fold(k);
			const uint32_t b = s / bsz;
			CHECK(b == bv_bucket(x, m1, nb) || b == bv_bucket(x, m2, nb),
			      "table %u: key %08x in bucket %u, not %u or %u", tbl, k[0], b,
			      bv_bucket(x, m1, nb), bv_bucket(x, m2, nb));
			++keys;
		}
	}

	// key words of a (possibly joint) table: the CoS slot in spare bits of
	// a one-word key, or appended
	static uint32_t joint_nk(uint32_t nk, uint32_t flags)
	{
		return (flags & BVJ_APPEND) ? nk + 1u : nk;
	}

	void block(uint32_t o)
	{
		const uint32_t *hot = p.w.data() + p.w[DH_HOT_OFF];
		const uint32_t *b = hot + o;
		const uint32_t mode = b[0] & 0xffu;
		CHECK(mode <= 4u, "block %u: mode %u", o, mode);
		if (mode == 0u) {   // direct: shared record b[2], nb b[4], table b[5], m1, m2
			table(joint_nk(hot[b[2] + 1u], b[1]), b[4], b[5], b[6], b[7]);
			return;
		}
		const uint32_t ncls = b[1] & 0xffu;
		CHECK(ncls >= 1 && ncls <= BV_MAX_CLS, "block %u: %u classes", o, ncls);
		for (uint32_t c = 0; c < ncls && !g_bad; ++c) {
			const uint32_t *r = b + 8u + BV_CLS_WORDS * c;
			table(joint_nk(r[1], mode == 2u ? r[13] : 0u), r[9], r[10], r[11], r[12]);
		}
	}

	void program()
	{
		const uint32_t *w = p.w.data();
		const uint32_t *hot = w + w[DH_HOT_OFF];
		for (uint32_t s = 0; s < w[DH_NCOS] && !g_bad; ++s) {
			const uint32_t bv = hot[COS_WORDS * s + C_BV];
			if (bv >> 31) {   // a chain of blocks: next block in header word 0
				for (uint32_t o = bv & C_BV_OFF; o && !g_bad; o = hot[o] >> 8)
					block(o);
			} else if (bv & C_BV_OFF) {
				block(bv & C_BV_OFF);
			}
		}
	}
};

static void run(const char *name, const char *kname, const std::vector<uint8_t> &blob,
		const MiAsmKnobs &kn)
{
	MiProgram p;
	const int rc = mi_asm_compile(blob.data(), blob.size(), kn, p);
	CHECK(rc == 0, "%s %s: mi_asm_compile %d", name, kname, rc);
	if (rc)
		return;
	CHECK(p.w.size() == p.w[DH_TOTAL] && p.w[DH_MAGIC] == DEV_MAGIC &&
	      p.w[DH_HOT_OFF] + p.hot_words <= p.w.size(), "%s %s: header", name, kname);
	Probe pr{ p, {}, 0, 0 };
	pr.program();
	std::string inst, src;
	if (p.spec_mode >= 0 || !p.plan.empty())
		src = mi_asm_spec_program(p, 16, true, false, inst);
	printf("%s %s words=%zu hot=%u tree=%d flat=%d spec=%d plan=", name, kname, p.w.size(),
	       p.hot_words, (int)p.tree, p.flat_mode, p.spec_mode);
	for (size_t i = 0; i < p.plan.size(); ++i)
		printf("%s%u", i ? "," : "", p.plan[i]);
	printf(" fnv=%016llx tables=%zu keys=%zu specfnv=%016llx\n",
	       (unsigned long long)fnv1a(p.w.data(), p.w.size() * sizeof(uint32_t)), pr.tables, pr.keys,
	       (unsigned long long)(src.empty() ? 0 : fnv1a(src.data(), src.size())));
}

static bool read_file(const char *path, std::vector<uint8_t> &out)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		return false;
	uint8_t buf[4096];
	for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
		out.insert(out.end(), buf, buf + n);
	fclose(f);
	return true;
}

// Every malformed table is refused before any index is followed.  Each is an
// exact-size heap copy, so a read past it is a sanitiser report.
static void hostile(const std::vector<uint8_t> &good)
{
	const MiAsmKnobs kn;
	MiProgram p;
	auto refused = [&](const char *what, const uint8_t *b, size_t n) {
		std::vector<uint8_t> copy(b, b + n);
		const int rc = mi_asm_compile(n ? copy.data() : nullptr, n, kn, p);
		CHECK(rc == -EINVAL, "hostile %s: %d", what, rc);
	};
	auto corrupt = [&](const char *what, const std::function<void(uint8_t *)> &f) {
		std::vector<uint8_t> b(good);
		f(b.data());
		refused(what, b.data(), b.size());
	};
	CHECK(mi_asm_compile(good.data(), good.size(), kn, p) == 0, "hostile: the blob itself");
	const mi_tbl_hdr_t *gh = (const mi_tbl_hdr_t *)good.data();
	CHECK(gh->num_cos && gh->num_rules && gh->num_terms && gh->default_cos >= 0,
	      "hostile: needs a table with CoS, rules, terms and a default CoS");
	if (g_bad)
		return;
	for (size_t n = 0; n < sizeof(mi_tbl_hdr_t); ++n)
		refused("truncated header", good.data(), n);
	refused("one byte short", good.data(), good.size() - 1);
	{
		std::vector<uint8_t> b(good);
		b.push_back(0);
		refused("one byte long", b.data(), b.size());
	}
	auto H = [](uint8_t *b) { return (mi_tbl_hdr_t *)b; };
	auto CS = [&](uint8_t *b) { return (mi_cos_t *)(b + H(b)->cos_off); };
	auto RS = [&](uint8_t *b) { return (mi_rule_t *)(b + H(b)->rule_off); };
	auto TS = [&](uint8_t *b) { return (mi_term_t *)(b + H(b)->term_off); };
	corrupt("total_bytes + 1", [&](uint8_t *b) { H(b)->total_bytes += 1; });
	corrupt("total_bytes - 1", [&](uint8_t *b) { H(b)->total_bytes -= 1; });
	corrupt("num_cos 257", [&](uint8_t *b) { H(b)->num_cos = 257; });
	corrupt("CoS rules past num_rules", [&](uint8_t *b) {
		mi_cos_t &c = CS(b)[H(b)->default_cos];
		c.rule_begin = H(b)->num_rules - c.num_rules + 1u;
	});
	corrupt("CoS rule_begin wraps", [&](uint8_t *b) { CS(b)[H(b)->default_cos].rule_begin = 0xFFFFFFFFu; });
	corrupt("num_queue 0", [&](uint8_t *b) { CS(b)[0].num_queue = 0; });
	corrupt("num_queue 33", [&](uint8_t *b) { CS(b)[H(b)->num_cos - 1].num_queue = 33; });
	corrupt("dst_cos = num_cos", [&](uint8_t *b) { RS(b)[H(b)->num_rules - 1].dst_cos = H(b)->num_cos; });
	corrupt("num_terms 9", [&](uint8_t *b) { RS(b)[0].num_terms = 9; });
	corrupt("term_begin past the end", [&](uint8_t *b) { RS(b)[0].term_begin = H(b)->num_terms; });
	corrupt("kind MI_K_COUNT", [&](uint8_t *b) { TS(b)[H(b)->num_terms - 1].kind = MI_K_COUNT; });
	corrupt("size 17", [&](uint8_t *b) { TS(b)[0].size = 17; });
	corrupt("default_cos = num_cos", [&](uint8_t *b) { H(b)->default_cos = (int32_t)H(b)->num_cos; });
	corrupt("default_cos -2", [&](uint8_t *b) { H(b)->default_cos = -2; });
	printf("hostile ok\n");
}

int main(int argc, char **argv)
{
	struct {
		const char *name;
		std::function<void(MiAsmKnobs &)> set;
	} const knobs[] = {
		{ "default", [](MiAsmKnobs &) {} },
		{ "no_bv", [](MiAsmKnobs &k) { k.no_bv = true; } },
		{ "div0", [](MiAsmKnobs &k) { k.div = 0; } },
		{ "div1", [](MiAsmKnobs &k) { k.div = 1; } },
		{ "no_wide", [](MiAsmKnobs &k) { k.no_wide = true; } },
		{ "no_cand1", [](MiAsmKnobs &k) { k.no_cand1 = true; } },
		{ "no_portmerge", [](MiAsmKnobs &k) { k.no_portmerge = true; } },
		{ "no_flat", [](MiAsmKnobs &k) { k.no_flat = true; } },
		{ "no_joint", [](MiAsmKnobs &k) { k.no_joint = true; } },
		{ "no_plan", [](MiAsmKnobs &k) { k.no_plan = true; } },
	};
	bool hostile_first = false;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "--hostile")) {
			hostile_first = true;
			continue;
		}
		std::vector<uint8_t> blob;
		CHECK(read_file(argv[i], blob), "cannot read %s", argv[i]);
		if (g_bad)
			break;
		const char *name = strrchr(argv[i], '/') ? strrchr(argv[i], '/') + 1 : argv[i];
		for (auto &k : knobs) {
			MiAsmKnobs kn;
			k.set(kn);
			run(name, k.name, blob, kn);
		}
		if (hostile_first) {
			hostile(blob);
			hostile_first = false;
		}
	}
	return g_bad ? 1 : 0;
}
