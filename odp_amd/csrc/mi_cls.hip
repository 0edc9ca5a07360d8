// mi_cls.hip -- host side of the MI355X packet parse + PMR classify path: the
// C ABI declared in include/mi_cls.h (contexts, rule loads, launches,
// host-batch staging, statistics).  The rule program is assembled by
// mi_cls_asm.cpp into the encoding of mi_cls_prog.h, specialised kernels are
// compiled and loaded by mi_cls_spec.cpp; the kernel itself is in
// mi_cls_dev.h, instantiated per block shape in mi_cls_k4/8/12/16.hip.
#include "mi_cls_dev.h"

#include "mi_cls_asm.h"
#include "mi_cls_spec.h"

#include <errno.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

// ------------------------------------------------------------------- host
struct mi_cls_ctx {
	int device;
	uint32_t *d_dev;         // assembled device rule program
	size_t dev_cap;          // bytes
	int loaded;
	MiProgram prog;          // the loaded program: host words and what kernels it runs
	int wpb;                 // forced waves per block (MI_CLS_WPB at load), 0 = auto
	uint32_t opt;            // pktin options (mi_cls_pktin_opt_set)
	unsigned long long *d_stats;
	uint32_t *d_hint;        // window hint word (KArgs.hint)
	uint32_t seq;            // launches so far
	int stats_on;
	uint32_t stats_mask[8];
	int num_cu;
	// host-batch staging (mi_cls_classify_host)
	hipStream_t stream;
	hipStream_t dstream;     // receive delivery (mi_cls_deliver_submit)
	uint32_t *h_off;         // pinned: rebased descriptors of a slice
	mi_cls_result_t *h_out;  // pinned: records of a slice (multi-GPU)
	uint8_t *d_pk;
	size_t pk_cap;
	uint32_t *d_off;
	uint16_t *d_len;
	mi_cls_result_t *d_out;
	uint32_t n_cap;
	// submitted host batches (mi_cls_classify_host_submit): completion
	// events in a ring, tickets numbered from 1
	hipEvent_t ev[8];
	uint64_t ev_done[8] = { 0 };   // per slot: the last ticket known complete
	uint8_t *d_rx;                 // receive chain: per ticket slot, its mi_cls_rxdev_t arrays
	const void *tab_src[8];        // per ticket slot: the table its copy was taken of,
	uint64_t tab_stamp[8];         // and that table's stamp
	mi_cls_rxtab_t *h_tab;         // per ticket slot: page-locked snapshot the copy reads
	uint64_t submitted;
	// the enqueue plan (mi_cls_enq_plan), made by its first call: the scratch
	// per record (enq_cap of them) and of fixed size, the table's page-locked
	// snapshot and whose copy the device holds, the last plan's end and stream
	uint8_t *d_enq = nullptr, *d_enq_fix = nullptr;
	size_t enq_cap = 0;
	mi_cls_enq_tab_t *h_enq_tab = nullptr;
	const void *enq_tab_src = nullptr;
	uint64_t enq_tab_stamp = 0;
	hipEvent_t enq_ev = nullptr;
	hipStream_t enq_last = nullptr;
	bool enq_used = false;
	// the run plan (mi_cls_enq_runs), likewise: the scratch per record (run_cap
	// of them) and of fixed size, the staged form's seq and runs (run_st_cap
	// bytes), the two tables' snapshot and whose copies the device holds
	uint8_t *d_run = nullptr, *d_run_fix = nullptr, *d_run_st = nullptr;
	size_t run_cap = 0, run_st_cap = 0;
	uint8_t *h_run_tab = nullptr;
	const void *run_tab_src[2] = { nullptr, nullptr };
	uint64_t run_tab_stamp[2] = { 0, 0 };
	hipEvent_t run_ev = nullptr;
	hipStream_t run_last = nullptr;
	bool run_used = false;
	// the pool plan (mi_cls_pool_plan), likewise: the scratch of fixed size, the
	// staged form's own, dec and idx (pool_st_cap records), the table's snapshot
	// and whose copy the device holds
	uint8_t *d_pool_fix = nullptr, *d_pool_st = nullptr;
	size_t pool_st_cap = 0;
	mi_cls_pool_tab_t *h_pool_tab = nullptr;
	const void *pool_tab_src = nullptr;
	uint64_t pool_tab_stamp = 0;
	hipEvent_t pool_ev = nullptr;
	hipStream_t pool_last = nullptr;
	bool pool_used = false;
	// the pool move (mi_cls_pool_move), likewise: the scratch of fixed size (the
	// table and dst_queue, the counters, the staged form's out), the staged
	// form's dec, idx, got, pk and ent (move_st_cap entries), the table's
	// snapshot and whose copy the device holds
	uint8_t *d_move_fix = nullptr, *d_move_st = nullptr;
	size_t move_st_cap = 0;
	uint8_t *h_move_tab = nullptr;
	const void *move_tab_src = nullptr;
	uint64_t move_tab_stamp = 0;
	hipEvent_t move_ev = nullptr;
	hipStream_t move_last = nullptr;
	bool move_used = false;
	// the vector fill (mi_cls_vec_fill), likewise: the scratch of fixed size
	// (the run table, the count matrix, the counters, the staged form's out),
	// the scratch per run (vec_cap of them), the staged form's arrays in one
	// buffer (vec_st_cap bytes), the run table's snapshot and whose copy the
	// device holds
	uint8_t *d_vec_fix = nullptr, *d_vec = nullptr, *d_vec_st = nullptr;
	size_t vec_cap = 0, vec_st_cap = 0;
	uint8_t *h_vec_tab = nullptr;
	const void *vec_tab_src = nullptr;
	uint64_t vec_tab_stamp = 0;
	hipEvent_t vec_ev = nullptr;
	hipStream_t vec_last = nullptr;
	bool vec_used = false;
	// program-specialised flat kernel for the loaded program (null: none)
	std::shared_ptr<SpecCode> spec;
	uint32_t batch_hint = 0; // largest batch per call (mi_cls_batch_hint), 0: unknown
	int spec_nw;             // its block shape
	bool spec_lt;
	bool spec_ck;            // the pktin-option (checksum) instantiation
	hipFunction_t spec_fn;   // loaded on this device (null: not yet)
	// the instantiation of the last launch (mi_cls_last_launch)
	uint32_t last[MI_CLS_LAUNCH_INFO_WORDS];
};

#define HIP_OK(x) do { if ((x) != hipSuccess) return -EIO; } while (0)
// one ticket slot's receive-chain arrays in HBM (mi_cls_rxdev_t): records,
// decisions, queue handles, lengths, pools, the table
#define RX_OFF_DEC ((size_t)MI_CLS_DLV_GROUP_MAX * sizeof(mi_cls_result_t))
#define RX_OFF_DQ (RX_OFF_DEC + (size_t)MI_CLS_DLV_GROUP_MAX * 4u)
#define RX_OFF_LEN (RX_OFF_DQ + (size_t)MI_CLS_DLV_GROUP_MAX * 8u)
#define RX_OFF_PP (RX_OFF_LEN + (size_t)MI_CLS_DLV_GROUP_MAX * 2u)
#define RX_OFF_TAB (RX_OFF_PP + (size_t)MI_CLS_DLV_GROUP_MAX)
#define RX_SLOT_BYTES ((RX_OFF_TAB + sizeof(mi_cls_rxtab_t) + 255u) & ~(size_t)255u)

// The calling thread's current device, set only when it differs (the
// receive path submits on one device per call)
static hipError_t set_device(int dev)
{
	int cur = -1;
	if (hipGetDevice(&cur) == hipSuccess && cur == dev)
		return hipSuccess;
	return hipSetDevice(dev);
}


extern "C" int mi_cls_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

// Resolve every kernel instantiation of the library on `device` (current
// device) once per process: each code object of the fat binary is loaded
// here, before the first launch, instead of on the first launch that picks
// one of its kernels -- which could come after program-specialised modules
// were loaded, late in the process's life (round 3's bench abort came on the
// first launch of a tree kernel after three specialised modules).
static int preload_kernels(int device)
{
	static std::mutex &mu = *new std::mutex;
	static std::set<int> &done = *new std::set<int>;
	std::lock_guard<std::mutex> g(mu);
	if (done.count(device))
		return 0;
	KArgs a;
	memset(&a, 0, sizeof(a));
	int bad = 0;
	auto chk = [&bad](int rc) {
		if (rc && rc != -ENOSYS)   // -ENOSYS: a variant build without that unit
			bad = rc;
	};
	for (int lt = 0; lt < 2; ++lt)
		for (int div = 0; div < 2; ++div) {
			chk(mi_cls_launch_k4(lt, div, 0, 0, nullptr, a));
			chk(mi_cls_launch_k8(lt, div, 0, 0, nullptr, a));
			chk(mi_cls_launch_k12(lt, div, 0, 0, nullptr, a));
			chk(mi_cls_launch_k16(lt, div, 0, 0, nullptr, a));
			chk(mi_cls_launch_ck(4, lt, div, 0, 0, nullptr, a));
			if (lt)
				chk(mi_cls_launch_ck(16, lt, div, 0, 0, nullptr, a));
		}
	for (int nw : { 4, 12, 16 })
		for (int fm : { 0, 2, 3, 4 })
			chk(mi_cls_launch_flat(nw, fm, 0, 0, nullptr, a));
	mi_cls_dlv_args_t da;
	memset(&da, 0, sizeof(da));
	chk(mi_cls_launch_deliver(0, nullptr, da));
	mi_cls_rxc_args_t ra;
	memset(&ra, 0, sizeof(ra));
	chk(mi_cls_launch_rx_chain(nullptr, ra, mi_cls_rxdev_t{}, true));
	chk(mi_cls_launch_rx_stage(nullptr, ra, mi_cls_rxdev_t{}, 0, true));
	chk(mi_cls_launch_tx(0, nullptr, TxArgs{}));
	chk(mi_cls_launch_tx_hash(true, 0, nullptr, TxHashArgs{}));
	chk(mi_cls_launch_tx_hash(false, 0, nullptr, TxHashArgs{}));
	for (uint32_t proto : { MI_CLS_PROTO_ETH, MI_CLS_PROTO_IPV4, MI_CLS_PROTO_IPV6 })
		for (int ck = 0; ck < 2; ++ck)
			chk(mi_cls_launch_parse(proto, ck != 0, 0, nullptr, ParseArgs{}));
	chk(mi_cls_launch_lso(0, nullptr, LsoArgs{}));
	chk(mi_cls_launch_enq(nullptr, EnqArgs{}, 0, true));
	chk(mi_cls_launch_run(nullptr, RunArgs{}, true));
	chk(mi_cls_launch_pool(nullptr, PoolArgs{}, true));
	chk(mi_cls_launch_move(nullptr, MoveArgs{}, true));
	chk(mi_cls_launch_vec(nullptr, VecArgs{}, true));
	if (bad)
		return bad;
	done.insert(device);
	return 0;
}

extern "C" int mi_cls_ctx_create(int device, mi_cls_ctx_t **out)
{
	if (!out)
		return -EINVAL;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
		return -ENODEV;
	mi_cls_ctx_t *c = new (std::nothrow) mi_cls_ctx_t();
	if (!c)
		return -ENOMEM;
	c->device = device;
	int cur = 0;
	(void)hipGetDevice(&cur);
	if (hipSetDevice(device) != hipSuccess) {
		delete c;
		return -EIO;
	}
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess)
		c->num_cu = prop.multiProcessorCount;
	else
		c->num_cu = 256;
	if (preload_kernels(device) != 0) {
		fprintf(stderr, "mi_cls: kernels could not be loaded on device %d\n", device);
		delete c;
		(void)hipSetDevice(cur);
		return -EIO;
	}
	if (hipMalloc((void **)&c->d_stats, MAX_STATS_COS * sizeof(unsigned long long)) != hipSuccess ||
	    hipMemset(c->d_stats, 0, MAX_STATS_COS * sizeof(unsigned long long)) != hipSuccess ||
	    hipMalloc((void **)&c->d_hint, sizeof(uint32_t)) != hipSuccess ||
	    hipMemset(c->d_hint, 0, sizeof(uint32_t)) != hipSuccess) {
		delete c;
		(void)hipSetDevice(cur);
		return -ENOMEM;
	}
	// the host-batch and delivery streams and the ticket ring's events are
	// made here, with the context, not by the first receive burst: a stream
	// creation takes milliseconds (it showed as ~7 ms of a 65 ms receive run)
	bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
		  hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking) == hipSuccess;
	for (int i = 0; i < 8 && ok; ++i)
		ok = hipEventCreateWithFlags(&c->ev[i], hipEventDisableTiming) == hipSuccess;
	ok = ok && hipMalloc((void **)&c->d_rx, 8 * RX_SLOT_BYTES) == hipSuccess;
	ok = ok && hipHostMalloc((void **)&c->h_tab, 8 * sizeof(mi_cls_rxtab_t), hipHostMallocDefault) ==
			   hipSuccess;
	if (!ok) {
		(void)hipSetDevice(cur);
		mi_cls_ctx_destroy(c);
		return -EIO;
	}
	(void)hipSetDevice(cur);
	*out = c;
	return 0;
}

extern "C" int mi_cls_ctx_destroy(mi_cls_ctx_t *c)
{
	if (!c)
		return -EINVAL;
	(void)hipSetDevice(c->device);
	if (c->d_dev)
		(void)hipFree(c->d_dev);
	if (c->d_stats)
		(void)hipFree(c->d_stats);
	if (c->d_hint)
		(void)hipFree(c->d_hint);
	if (c->stream) {
		(void)hipStreamSynchronize(c->stream);
		(void)hipStreamDestroy(c->stream);
	}
	if (c->dstream) {
		(void)hipStreamSynchronize(c->dstream);
		(void)hipStreamDestroy(c->dstream);
	}
	for (int i = 0; i < 8; ++i) {
		if (c->ev[i])
			(void)hipEventDestroy(c->ev[i]);
	}
	if (c->enq_ev) {
		(void)hipEventSynchronize(c->enq_ev);
		(void)hipEventDestroy(c->enq_ev);
	}
	(void)hipFree(c->d_enq);
	(void)hipFree(c->d_enq_fix);
	if (c->h_enq_tab)
		(void)hipHostFree(c->h_enq_tab);
	if (c->run_ev) {
		(void)hipEventSynchronize(c->run_ev);
		(void)hipEventDestroy(c->run_ev);
	}
	(void)hipFree(c->d_run);
	(void)hipFree(c->d_run_fix);
	(void)hipFree(c->d_run_st);
	if (c->h_run_tab)
		(void)hipHostFree(c->h_run_tab);
	if (c->pool_ev) {
		(void)hipEventSynchronize(c->pool_ev);
		(void)hipEventDestroy(c->pool_ev);
	}
	(void)hipFree(c->d_pool_fix);
	(void)hipFree(c->d_pool_st);
	if (c->h_pool_tab)
		(void)hipHostFree(c->h_pool_tab);
	if (c->move_ev) {
		(void)hipEventSynchronize(c->move_ev);
		(void)hipEventDestroy(c->move_ev);
	}
	(void)hipFree(c->d_move_fix);
	(void)hipFree(c->d_move_st);
	if (c->h_move_tab)
		(void)hipHostFree(c->h_move_tab);
	if (c->vec_ev) {
		(void)hipEventSynchronize(c->vec_ev);
		(void)hipEventDestroy(c->vec_ev);
	}
	(void)hipFree(c->d_vec_fix);
	(void)hipFree(c->d_vec);
	(void)hipFree(c->d_vec_st);
	if (c->h_vec_tab)
		(void)hipHostFree(c->h_vec_tab);
	(void)hipFree(c->d_rx);
	if (c->h_tab)
		(void)hipHostFree(c->h_tab);
	(void)hipFree(c->d_pk);
	(void)hipFree(c->d_off);
	(void)hipFree(c->d_len);
	(void)hipFree(c->d_out);
	(void)hipHostFree(c->h_off);
	(void)hipHostFree(c->h_out);
	delete c;
	return 0;
}

// Host-only introspection of the device encoding a table assembles into (no
// device needed): info[0] total words, [1] hot-region words, [2] CoS with a
// classification block, [3..6] blocks per mode (direct, candidate, bitmap,
// wide), [7] 1 if the program is a tree (DIV kernel), [8] single-candidate
// blocks, [9] flat engine + 1 (0: not flat), [10] chains of blocks, [11],
// [12] members of direct and bitmap joint groups.  Tests and tools use it to
// check the engine choice on the CPU.
extern "C" int mi_cls_program_info(const void *tbl, size_t bytes, uint32_t *info, uint32_t n)
{
	if (!info || n < 9)
		return -EINVAL;
	MiProgram p;
	const int rc = mi_asm_compile(tbl, bytes, mi_asm_knobs_from_env(), p);
	if (rc)
		return rc;
	const uint32_t *w = p.w.data();
	memset(info, 0, n * sizeof(uint32_t));
	info[0] = (uint32_t)p.w.size();
	info[1] = p.hot_words;
	const uint32_t *hot = w + w[DH_HOT_OFF];
	info[7] = p.tree;
	for (uint32_t s = 0; s < w[DH_NCOS]; ++s) {
		const uint32_t bv = hot[COS_WORDS * s + C_BV] & C_BV_OFF;
		if (bv) {
			info[2]++;
			const uint32_t md = hot[bv] & 0xffu;
			info[md == 4u ? 8u : 3u + (md & 3u)]++;
			if (n > 10 && (hot[COS_WORDS * s + C_BV] >> 31))
				info[10]++;
			const uint32_t gid = (hot[COS_WORDS * s + C_BV] >> 24) & 0x7fu;
			if (n > 12 && gid && info[7])
				info[hot[hot[w[DH_JOINT] + gid - 1u]] == 0u ? 11u : 12u]++;
		}
	}
	if (n > 9)
		info[9] = (uint32_t)(p.flat_mode + 1);
	return 0;
}

static void spec_setup(mi_cls_ctx_t *c);

extern "C" int mi_cls_rules_load(mi_cls_ctx_t *c, const void *tbl, size_t bytes, void *stream)
{
	if (!c)
		return -EINVAL;
	const MiAsmKnobs kn = mi_asm_knobs_from_env();
	MiProgram p;
	const int rc = mi_asm_compile(tbl, bytes, kn, p);
	if (rc)
		return rc;
	// host batches and receive chains still in flight classify with the
	// rules they were submitted under
	if ((c->stream && hipStreamSynchronize(c->stream) != hipSuccess) ||
	    (c->dstream && hipStreamSynchronize(c->dstream) != hipSuccess))
		return -EIO;
	{
		const char *e = getenv("MI_CLS_WPB");
		c->wpb = e ? atoi(e) : 0;
	}
	if (kn.verbose)
		fprintf(stderr, "mi_cls: program %zu words, hot region %u words\n", p.w.size(), p.hot_words);
	const size_t nbytes = p.w.size() * sizeof(uint32_t);
	HIP_OK(hipSetDevice(c->device));
	if (nbytes > c->dev_cap) {
		// the old program may still be read by in-flight launches
		if (c->d_dev) {
			HIP_OK(hipStreamSynchronize((hipStream_t)stream));
			(void)hipFree(c->d_dev);
			c->d_dev = nullptr;
		}
		size_t cap = nbytes < 4096 ? 4096 : nbytes;
		if (hipMalloc((void **)&c->d_dev, cap) != hipSuccess)
			return -ENOMEM;
		c->dev_cap = cap;
	}
	// stream-ordered after earlier launches; synchronous w.r.t. the host
	// words, which the copy must not outlive unchanged
	HIP_OK(hipMemcpyAsync(c->d_dev, p.w.data(), nbytes, hipMemcpyHostToDevice, (hipStream_t)stream));
	HIP_OK(hipStreamSynchronize((hipStream_t)stream));
	c->prog = std::move(p);
	c->loaded = 1;
	spec_setup(c);
	return 0;
}

// Block shape of a launch.  One wave per 64-packet tile in flight; the grid
// covers the resident capacity (blocks per CU: 4 = the VGPR-bound occupancy
// of 4 waves/SIMD, fewer when the LDS copy of the hot region does not leave
// room) and each wave loops over its tiles with the load pipeline.
// MI_CLS_BLOCKS_PER_CU overrides the block count, MI_CLS_LDS_HOT_MAX (bytes)
// the largest hot region copied into LDS.
// Block shape: 4-wave blocks, four per CU, each with its own LDS copy of the
// hot region when it is small (<= MI_CLS_LDS_HOT_MAX); otherwise one block per
// CU of 16, 12 or 8 waves sharing one copy -- the most waves whose windows
// leave room for it; otherwise 4-wave blocks reading the hot region from HBM.
// MI_CLS_WPB=4|8|12|16 forces a shape (A/B runs).
struct Shape {
	int nw;          // waves per block
	bool lt;         // hot region copied into LDS
	size_t dyn;      // dynamic LDS bytes
	int per_cu;      // blocks per CU
};

static Shape pick_shape(const mi_cls_ctx_t *c, uint32_t opt)
{
	static int per_cu_env = -2, hot_max = -1;
	if (per_cu_env == -2) {
		const char *e = getenv("MI_CLS_BLOCKS_PER_CU");
		per_cu_env = e ? atoi(e) : -1;
		e = getenv("MI_CLS_LDS_HOT_MAX");
		hot_max = e ? atoi(e) : 20 * 1024;
	}
	const int wpb_env = c->wpb;
	const size_t LDS_CU = 160u * 1024u;
	const size_t hot_bytes = (((size_t)c->prog.hot_words + 3u) & ~(size_t)3u) * sizeof(uint32_t);
	// static LDS of a block: windows, stats histogram, L4 table (+ the
	// CRC-32C tables of the pktin-option kernels)
	const size_t st_ck = opt != 0 ? CRC_WORDS : 0;
	auto st_of = [st_ck](int w) {
		// (+ 1 word: the block's tile counter)
		return sizeof(uint32_t) * ((size_t)w * RS * WROWS + MAX_STATS_COS + 256 + 1 + st_ck);
	};
	const bool small = (long)hot_bytes <= (long)hot_max;
	const bool full4 = small && 4 * (st_of(4) + hot_bytes) <= LDS_CU;
	// One block of 16 waves per CU when its windows and the hot region fit:
	// the block's tiles are dealt to its waves by an LDS counter, so a CU's
	// 16 waves share its work (mi_cls_kernel); 4-wave blocks balance only
	// among their 4 (configs 2 / 3 64 B: 18.4 -> 17.8, 20.9 -> 19.5 us;
	// profiles/r06_tile_queue_ab.txt).  Otherwise 4-wave blocks with their
	// own copy (small regions), else 12 or 8 waves.
	// Batches of fewer than two tiles per wave of one 16-wave block per CU
	// (receive bursts, mi_cls_batch_hint) are spread over more CUs in 4-wave
	// blocks: a 4096-frame burst then runs on 16 CUs, not 4 (pcap receive
	// 45.9 -> 46.7, loop 38.1 -> 42.8 Mpkt/s; profiles/r06_rx_ab.txt).
	const bool small_batch = c->batch_hint != 0 &&
				 c->batch_hint < 2u * (uint32_t)c->num_cu * 16u * WAVE;
	int nw = 4;
	bool lt = full4;
	for (int w : { 16, 12, 8 })
		if (st_of(w) + hot_bytes <= LDS_CU) {
			nw = w;
			lt = true;
			break;
		}
	if ((nw == 8 || small_batch) && full4) {
		nw = 4;   // 4-wave blocks, four per CU
		lt = true;
	}
	if (wpb_env == 4 || wpb_env == 8 || wpb_env == 12 || wpb_env == 16) {
		nw = wpb_env;
		lt = nw == 4 ? small && st_of(4) + hot_bytes <= LDS_CU : st_of(nw) + hot_bytes <= LDS_CU;
		if (nw != 4 && nw != 16 && !lt)
			nw = 16;   // 8 / 12-wave blocks exist for LDS-resident hot regions only
	}
	if (opt != 0 && nw != 4) {
		// the pktin-option kernels exist as 4-wave blocks and as 16-wave
		// blocks with the hot region in LDS
		nw = 16;
		lt = st_of(16) + hot_bytes <= LDS_CU;
		if (!lt)
			nw = 4;
	}
	const size_t lds_block = st_of(nw) + (lt ? hot_bytes : 0);
	int per_cu = (int)(LDS_CU / lds_block);
	const int occ = MIN_WAVES_PER_EU;   // waves/SIMD the register budget allows
	if (per_cu > occ * 4 / nw)
		per_cu = occ * 4 / nw;
	if (per_cu_env > 0)
		per_cu = per_cu_env;
	if (per_cu < 1)
		per_cu = 1;
	return Shape{ nw, lt, lt ? hot_bytes : 0, per_cu };
}

// ------------------------------------------------ program-specialised kernels
// A flat program (decided on the default CoS in one round) or a CoS tree
// with a plan gets its own kernel, compiled in the background from the text
// the assembler writes (mi_cls_asm.cpp) by the compile manager
// (mi_cls_spec.cpp); launches use the generic kernels until it is loaded.

// MI_CLS_DUMP_SPEC=<file>: the hipRTC program, for inspection
static void dump_spec(const std::string &src)
{
	const char *dp = getenv("MI_CLS_DUMP_SPEC");
	FILE *f = dp ? fopen(dp, "w") : nullptr;
	if (f) {
		fputs(src.c_str(), f);
		fclose(f);
	}
}

// Host-only check (no device): compile the specialised kernel of a table's
// program synchronously.  0 = compiled, 1 = the program is not flat, <0 =
// error (-ENOEXEC: hipRTC failed; MI_CLS_VERBOSE prints its log).
extern "C" int mi_cls_spec_compile(const void *tbl, size_t bytes, int nw)
{
	MiProgram p;
	const int rc = mi_asm_compile(tbl, bytes, mi_asm_knobs_from_env(), p);
	if (rc)
		return rc;
	if (nw != 4 && nw != 12 && nw != 16)
		return -EINVAL;
	if (p.spec_mode < 0 && p.plan.empty())
		return 1;
	std::string inst;
	const std::string src = mi_asm_spec_program(p, nw, true, false, inst);
	dump_spec(src);
	return mi_spec_compile_now(src, inst);
}

static bool spec_enabled(void)
{
	const char *e = getenv("MI_CLS_JIT");
	return !(e && e[0] == '0');
}

// After a rule load (or a change of the pktin options or the batch hint):
// the specialisation of the loaded program (compiled in the background
// unless cached), or none.
static void spec_setup(mi_cls_ctx_t *c)
{
	c->spec.reset();
	c->spec_fn = nullptr;
	// Flat programs: the flat kernel with its block compiled in (1-2 s of
	// hipRTC).  CoS trees whose levels are joint groups (tree plan): the
	// default CoS's block and the plan's groups compiled in, no generic
	// per-lane engines (round 3 compiled only the first round into the
	// general kernel: ~100 s of hipRTC and 1.7x slower on config 5).  With
	// pktin options on, flat programs and tree plans get the option kernel
	// (checksums) with the block / plan compiled in, in the option kernels'
	// block shape.
	const bool ck = c->opt != 0;
	const bool flat = c->prog.spec_mode >= 0;
	if ((!flat && c->prog.plan.empty()) || !spec_enabled())
		return;
	const Shape sh = pick_shape(c, c->opt);
	// (a tree plan's option kernel may read its hot region from HBM: config 5's
	// 52 KB region and the CRC tables leave 16-wave blocks no LDS for it)
	if (ck ? ((flat && !sh.lt) || (sh.nw != 4 && sh.nw != 16))
	       : flat ? (!sh.lt || (sh.nw != 4 && sh.nw != 12 && sh.nw != 16))
		      : (sh.nw != 4 && sh.nw != 8 && sh.nw != 12 && sh.nw != 16))
		return;
	std::string inst;
	const std::string src = mi_asm_spec_program(c->prog, sh.nw, flat ? true : sh.lt, ck, inst);
	dump_spec(src);
	c->spec = mi_spec_request(src, inst);
	c->spec_nw = sh.nw;
	c->spec_lt = sh.lt;
	c->spec_ck = ck;
}

// The context's specialisation on its device once compiled (wait: block
// until the compilation ends).  Returns the kernel, or null (still
// compiling, failed, dropped, or none; after a failure the context runs the
// generic kernel for this program).
static hipFunction_t spec_fn(mi_cls_ctx_t *c, bool wait)
{
	if (c->spec_fn || !c->spec)
		return c->spec_fn;
	hipFunction_t fn = nullptr;
	if (!mi_spec_function(*c->spec, c->device, wait, &fn))
		return nullptr;
	if (!fn)
		c->spec.reset();   // generic kernel for this program
	c->spec_fn = fn;
	return fn;
}


extern "C" int mi_cls_last_launch(const mi_cls_ctx_t *c, uint32_t *info, uint32_t n)
{
	if (!c || (!info && n))
		return -EINVAL;
	const uint32_t k = n < MI_CLS_LAUNCH_INFO_WORDS ? n : MI_CLS_LAUNCH_INFO_WORDS;
	memcpy(info, c->last, k * sizeof(uint32_t));
	return (int)k;
}

extern "C" int mi_cls_spec_wait(mi_cls_ctx_t *c)
{
	if (!c || !c->loaded)
		return -EINVAL;
	if (!c->spec)
		return 1;
	return spec_fn(c, true) ? 0 : 1;
}

extern "C" int mi_cls_classify(mi_cls_ctx_t *c, const uint8_t *pkts, const uint32_t *off,
			       const uint16_t *len, uint32_t n, mi_cls_result_t *out, void *stream)
{
	if (!c || !c->loaded)
		return -EINVAL;
	if (n == 0)
		return 0;
	if (!pkts || !off || !len || !out)
		return -EINVAL;
	if (((uintptr_t)out & 15u) != 0 || n > MI_CLS_MAX_BATCH)
		return -EINVAL;
	HIP_OK(hipSetDevice(c->device));
	KArgs a;
	a.pkts = pkts;
	a.off = off;
	a.len = len;
	a.n = n;
	a.dev = c->d_dev;
	a.out = out;
	a.stats = c->stats_on ? c->d_stats : nullptr;
	a.opt = c->opt;
	a.hint = c->d_hint;
	a.seq = ++c->seq;
	if (a.seq == 0u)   // wrapped: the hint word may equal seq - 1 by accident
		a.seq = c->seq = 2u;
	memcpy(a.stats_mask, c->stats_mask, sizeof(a.stats_mask));
	// the program's header words (the loaded program's host copy: what d_dev holds)
	memcpy(a.hdr, c->prog.w.data(), sizeof(a.hdr));
	const Shape sh = pick_shape(c, c->opt);
	const int nw = sh.nw;
	const bool lt = sh.lt;
	const bool div = c->prog.tree;
	const uint32_t bthreads = (uint32_t)nw * WAVE;
	uint32_t tiles = (n + bthreads - 1) / bthreads;
	uint32_t max_grid = (uint32_t)c->num_cu * (uint32_t)sh.per_cu;
	uint32_t grid = tiles < max_grid ? tiles : max_grid;
	const size_t dyn = sh.dyn;
	hipStream_t st = (hipStream_t)stream;
	int lrc;
	uint32_t *last = c->last;
	last[0] = (uint32_t)nw;
	last[1] = lt;
	last[2] = 0;
	last[3] = 0;
	last[4] = 0;
	last[5] = c->opt != 0;
	last[6] = grid;
	const bool spec_ok = c->spec && c->spec_ck == (c->opt != 0) && c->spec_nw == nw &&
			     c->spec_lt == lt && spec_fn(c, false);
	if (c->opt != 0 && spec_ok) {
		// the option kernel with the program's block (or tree plan) compiled in
		last[2] = c->prog.flat_mode < 0 && div;
		last[3] = (uint32_t)(c->prog.flat_mode + 1);
		last[4] = 1;
		void *args[] = { &a };
		lrc = hipModuleLaunchKernel(c->spec_fn, grid, 1, 1, (unsigned)bthreads, 1, 1,
					    (unsigned)dyn, st, args, nullptr) == hipSuccess ? 0 : -EIO;
	} else if (c->opt != 0) {
		last[2] = div;
		lrc = mi_cls_launch_ck(nw, lt, div, grid, dyn, st, a);
	} else if (spec_ok) {
		last[2] = c->prog.flat_mode < 0 && div;   // a tree plan
		last[3] = (uint32_t)(c->prog.flat_mode + 1);
		last[4] = 1;
		void *args[] = { &a };
		lrc = hipModuleLaunchKernel(c->spec_fn, grid, 1, 1, (unsigned)bthreads, 1, 1,
					    (unsigned)dyn, st, args, nullptr) == hipSuccess ? 0 : -EIO;
	} else if (c->prog.flat_mode >= 0 && c->prog.flat_mode != 1 && lt && (nw == 4 || nw == 12 || nw == 16)) {
		last[3] = (uint32_t)(c->prog.flat_mode + 1);
		lrc = mi_cls_launch_flat(nw, c->prog.flat_mode, grid, dyn, st, a);
	} else {
		last[2] = div;
		if (nw == 16)
			lrc = mi_cls_launch_k16(lt, div, grid, dyn, st, a);
		else if (nw == 12)
			lrc = mi_cls_launch_k12(lt, div, grid, dyn, st, a);
		else if (nw == 8)
			lrc = mi_cls_launch_k8(lt, div, grid, dyn, st, a);
		else
			lrc = mi_cls_launch_k4(lt, div, grid, dyn, st, a);
	}
	if (lrc)
		return lrc;
	if (hipGetLastError() != hipSuccess)
		return -EIO;
	return 0;
}

// ------------------------------------------------------------- host batches
// The steps classify, checksum insertion, parse and LSO share (DESIGN.md,
// "The host-batch contract"), each written once.

// Device address of page-locked host memory (hipHostMalloc /
// hipHostRegister), NULL for pageable memory.
// Page-locked allocations of mi_cls_host_alloc: start -> (bytes, device
// view - host address).  dev_view() answers from here without a runtime
// call (the receive path checks several buffers per burst).
struct HostRange {
	size_t bytes;
	ptrdiff_t delta;
};
static std::mutex g_hreg_mu;
static std::map<uintptr_t, HostRange> g_hreg;

static const void *dev_view_slow(const void *p)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) {
		(void)hipGetLastError();
		return nullptr;
	}
	if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer)
		return nullptr;
	return (const uint8_t *)a.devicePointer + ((const uint8_t *)p - (const uint8_t *)a.hostPointer);
}

static const void *dev_view(const void *p)
{
	{
		std::lock_guard<std::mutex> lk(g_hreg_mu);
		auto it = g_hreg.upper_bound((uintptr_t)p);
		if (it != g_hreg.begin()) {
			--it;
			if ((uintptr_t)p - it->first < it->second.bytes)
				return (const uint8_t *)p + it->second.delta;
		}
	}
	return dev_view_slow(p);
}

// Each pointer replaced by its device view, in order, up to the first one
// that is pageable: true when all of them are page-locked.
template <typename T> static bool dev_views(T *&p)
{
	const void *d = dev_view(p);
	return d ? (p = (T *)d, true) : false;
}
template <typename T, typename... U> static bool dev_views(T *&p, U *&...more)
{
	return dev_views(p) && dev_views(more...);
}

// What an entry point answers without a context
static int no_ctx(void)
{
	return mi_cls_device_count() > 0 ? -EINVAL : -ENODEV;
}

// Every frame lies inside the `bytes` of its buffer
static bool frames_inside(const uint32_t *off, const uint16_t *len, uint32_t n, size_t bytes)
{
	for (uint32_t i = 0; i < n; ++i)
		if ((size_t)off[i] + len[i] > bytes)
			return false;
	return true;
}

// The zero-copy condition: the kernels read a frame in 16-B pieces from its
// start, and every frame's last piece lies inside the caller's `lim` bytes
// (a batch that fails it is staged into the padded device buffer)
static bool frames_padded_inside(const uint32_t *off, const uint16_t *len, uint32_t n, size_t lim)
{
	for (uint32_t i = 0; i < n; ++i)
		if ((size_t)off[i] + (((size_t)len[i] + 15u) & ~(size_t)15u) > lim)
			return false;
	return true;
}

// The context's device staging buffers for a host batch of `need` frame bytes
// (padding included) and n entries, grown geometrically and kept across
// calls: d_pk, d_off, d_len, d_out (16 B per entry: records, or what the
// stg_* accessors below place there) and the pinned h_off / h_out.
static int stage_bufs(mi_cls_ctx_t *c, size_t need, uint32_t n)
{
	if ((need > c->pk_cap || n > c->n_cap) && c->submitted)
		HIP_OK(hipStreamSynchronize(c->stream));   // buffers of submitted batches
	if (need > c->pk_cap) {
		(void)hipFree(c->d_pk);
		c->d_pk = nullptr;
		size_t cap = need < (1u << 20) ? (1u << 20) : need + need / 2;
		if (hipMalloc((void **)&c->d_pk, cap) != hipSuccess)
			return c->pk_cap = 0, -ENOMEM;
		HIP_OK(hipMemset(c->d_pk, 0, cap));
		c->pk_cap = cap;
	}
	if (n > c->n_cap) {
		(void)hipFree(c->d_off);
		(void)hipFree(c->d_len);
		(void)hipFree(c->d_out);
		(void)hipHostFree(c->h_off);
		(void)hipHostFree(c->h_out);
		c->d_off = nullptr;
		c->d_len = nullptr;
		c->d_out = nullptr;
		c->h_off = nullptr;
		c->h_out = nullptr;
		uint32_t cap = n < 4096u ? 4096u : n + n / 2;
		if (hipMalloc((void **)&c->d_off, cap * sizeof(uint32_t)) != hipSuccess ||
		    hipMalloc((void **)&c->d_len, cap * sizeof(uint16_t)) != hipSuccess ||
		    hipMalloc((void **)&c->d_out, cap * sizeof(mi_cls_result_t)) != hipSuccess ||
		    hipHostMalloc((void **)&c->h_off, cap * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
		    hipHostMalloc((void **)&c->h_out, cap * sizeof(mi_cls_result_t), hipHostMallocDefault) != hipSuccess)
			return c->n_cap = 0, -ENOMEM;
		c->n_cap = cap;
	}
	return 0;
}

// Stage a batch up on the context's stream: staging buffers for `room` frame
// bytes (+ 64 of padding) and `entries` per-entry slots, then the `bytes` at
// `frames` to d_pk, the n offsets (less `rebase`, through h_off) to d_off and
// the n lengths to d_len.
static int stage_up(mi_cls_ctx_t *c, const uint8_t *frames, size_t bytes, size_t room, const uint32_t *off,
		    const uint16_t *len, uint32_t n, uint32_t entries, size_t rebase = 0)
{
	const int rc = stage_bufs(c, room + 64, entries);
	if (rc)
		return rc;
	if (rebase) {
		for (uint32_t i = 0; i < n; ++i)
			c->h_off[i] = off[i] - (uint32_t)rebase;
		off = c->h_off;
	}
	HIP_OK(hipMemcpyAsync(c->d_pk, frames, bytes, hipMemcpyHostToDevice, c->stream));
	HIP_OK(hipMemcpyAsync(c->d_off, off, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIP_OK(hipMemcpyAsync(c->d_len, len, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
	return 0;
}

// What the staged forms of checksum insertion and LSO place in the staging
// buffers beside frames, offsets and lengths (d_out has 16 B, d_len 2 B for
// each of n_cap entries).  Checksum, n entries: d_out = n_cap descriptors
// (8 B), then the done bytes.  LSO, 2n + nsegs entries: d_out = n descriptors
// (16 B), then the segment table (8 B each); d_len = n lengths, then n status
// bytes; d_pk = the sources, then, from a 256-B boundary, the destination
// (the same bytes when src == dst).
static mi_cls_tx_desc_t *stg_tx_desc(const mi_cls_ctx_t *c) { return (mi_cls_tx_desc_t *)c->d_out; }
static uint8_t *stg_tx_done(const mi_cls_ctx_t *c) { return (uint8_t *)(stg_tx_desc(c) + c->n_cap); }
// the flow hash (mi_cls_tx_hash_host), n entries: d_out = n_cap descriptors,
// then n_cap hash words, then the done bytes
static uint32_t *stg_txh_hash(const mi_cls_ctx_t *c) { return (uint32_t *)(stg_tx_desc(c) + c->n_cap); }
static uint8_t *stg_txh_done(const mi_cls_ctx_t *c) { return (uint8_t *)(stg_txh_hash(c) + c->n_cap); }
static mi_cls_lso_desc_t *stg_lso_desc(const mi_cls_ctx_t *c) { return (mi_cls_lso_desc_t *)c->d_out; }
static mi_cls_lso_seg_t *stg_lso_seg(const mi_cls_ctx_t *c, uint32_t n) { return (mi_cls_lso_seg_t *)(c->d_out + n); }
static uint8_t *stg_lso_st(const mi_cls_ctx_t *c, uint32_t n) { return (uint8_t *)(c->d_len + n); }
static size_t stg_lso_dst(bool same, size_t src_bytes) { return same ? 0 : (src_bytes + 255u) & ~(size_t)255u; }

// ---- the ticket ring: tickets numbered from 1, completion events in 8 slots
// Wait for ticket t (its slot still holds it): nothing if it was seen
// complete before, else a query, then a blocking wait only if it runs.
static int ring_wait(mi_cls_ctx_t *c, uint64_t t)
{
	if (c->ev_done[t % 8] == t)
		return 0;
	const hipError_t q = hipEventQuery(c->ev[t % 8]);
	if (q != hipSuccess &&
	    (q != hipErrorNotReady || hipEventSynchronize(c->ev[t % 8]) != hipSuccess))
		return -EIO;
	c->ev_done[t % 8] = t;
	return 0;
}

// Begin the context's next ticket t: its device current and its ring slot
// t % 8 free, that is ticket t - 8 complete (the submitter may now reuse the
// slot's own arrays).  A ticket already waited for needs no runtime call;
// otherwise a query, and a blocking wait only while it still runs.
static int ticket_begin(mi_cls_ctx_t *c, uint64_t *t)
{
	*t = c->submitted + 1;
	HIP_OK(set_device(c->device));
	return ring_wait(c, *t - 8);
}

// Commit ticket t: its event after what the submitter queued on stream `s`
static int ticket_commit(mi_cls_ctx_t *c, uint64_t t, hipStream_t s, uint64_t *ticket)
{
	HIP_OK(hipEventRecord(c->ev[t % 8], s));
	c->submitted = t;
	*ticket = t;
	return 0;
}

// The two forms of a checked host batch over its feature's `launch` (which
// queues the batch on the context's stream): the _host form (ticket NULL)
// waits for the stream, the _host_submit form commits a ticket.
template <typename L> static int host_run(mi_cls_ctx_t *c, uint64_t *ticket, L launch)
{
	uint64_t t = 0;
	int rc = ticket ? ticket_begin(c, &t) : 0;
	if (!rc)
		rc = launch();
	if (rc)
		return rc;
	if (ticket)
		return ticket_commit(c, t, c->stream, ticket);
	HIP_OK(hipStreamSynchronize(c->stream));
	return 0;
}

// Wait for a ticket of the ring (every feature's _host_wait)
static int host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	if (ticket > c->submitted)
		return -EINVAL;
	if (ticket == 0 || ticket + 8 <= c->submitted)
		return 0;   // nothing submitted, or its slot was reused (waited for then)
	HIP_OK(set_device(c->device));
	return ring_wait(c, ticket);
}

// ------------------------------------------------------- classify host batch
// Frames [lo, hi) of a host batch (the group entries give a slice) on the
// context's stream, nothing waited for: in place when frames, descriptors
// and records are page-locked and frames_padded_inside(lim), `lim` being the
// size of the caller's buffer at `pkts` -- only the header windows the
// kernel touches cross the host link then, not whole frames.  Otherwise
// staged, the descriptors rebased by lo.  The records go to `out` (any host
// memory) or, when out is NULL, to the context's pinned record buffer h_out
// (multi-GPU: no host wait per device).
static int host_launch(mi_cls_ctx_t *c, const uint8_t *pkts, size_t lo, size_t hi, size_t lim,
		       const uint32_t *off, const uint16_t *len, uint32_t n, mi_cls_result_t *out)
{
	HIP_OK(set_device(c->device));
	const uint8_t *zp = pkts;
	const uint32_t *zo = off;
	const uint16_t *zl = len;
	mi_cls_result_t *zr = out ? out : n <= c->n_cap ? c->h_out : nullptr;
	if (dev_views(zp, zo, zl) && frames_padded_inside(off, len, n, lim) && zr && dev_views(zr))
		return mi_cls_classify(c, zp, zo, zl, n, zr, c->stream);   // offsets stay relative to `pkts`
	int rc = stage_up(c, pkts + lo, hi - lo, hi - lo, off, len, n, n, lo);
	if (rc)
		return rc;
	rc = mi_cls_classify(c, c->d_pk, c->d_off, c->d_len, n, c->d_out, c->stream);
	if (rc)
		return rc;
	HIP_OK(hipMemcpyAsync(out ? out : c->h_out, c->d_out, n * sizeof(mi_cls_result_t),
			      hipMemcpyDeviceToHost, c->stream));
	return 0;
}

static int classify_host_check(const mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes, const uint32_t *off,
			       const uint16_t *len, uint32_t n, const mi_cls_result_t *out)
{
	if (!c || !c->loaded)
		return -EINVAL;
	if (n == 0)
		return 0;
	return pkts && off && len && out && frames_inside(off, len, n, bytes) ? 0 : -EINVAL;
}

extern "C" int mi_cls_classify_host(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes,
				    const uint32_t *off, const uint16_t *len, uint32_t n,
				    mi_cls_result_t *out)
{
	const int rc = classify_host_check(c, pkts, bytes, off, len, n, out);
	if (rc || n == 0)
		return rc;
	return host_run(c, nullptr, [&] { return host_launch(c, pkts, 0, bytes, bytes, off, len, n, out); });
}

// Submit a host batch without waiting (pipelined receive): the caller keeps
// pkts / off / len / out untouched until mi_cls_classify_host_wait(ticket).
extern "C" int mi_cls_classify_host_submit(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes,
					   const uint32_t *off, const uint16_t *len, uint32_t n,
					   mi_cls_result_t *out, uint64_t *ticket)
{
	if (!c || !c->loaded || !ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = classify_host_check(c, pkts, bytes, off, len, n, out);
	if (rc || n == 0)
		return rc;
	return host_run(c, ticket, [&] { return host_launch(c, pkts, 0, bytes, bytes, off, len, n, out); });
}

extern "C" int mi_cls_host_mapped(const void *p)
{
	return p && dev_view(p) == p ? 1 : 0;
}

// Receive delivery of a classified burst (mi_cls_kd.hip) on the context's
// delivery stream: the records were waited for by the host (it decided
// every frame from them), so nothing orders it after the classify stream,
// and the next burst's classification runs beside it.  Tickets share the
// context's ring with mi_cls_classify_host_submit.
extern "C" int mi_cls_deliver_submit(mi_cls_ctx_t *c, const mi_cls_dlv_args_t *a, uint64_t *ticket)
{
	if (!c || !a || !ticket)
		return -EINVAL;
	*ticket = 0;
	if (a->n == 0)
		return 0;
	if (!mi_cls_host_mapped(a->base) || !mi_cls_host_mapped(a->res) ||
	    !mi_cls_host_mapped(a->dlv) || !mi_cls_host_mapped(a->perm) || !mi_cls_host_mapped(a->gcnt) ||
	    a->layer < 1u || a->layer > 4u)
		return -EINVAL;
	if (a->n > MI_CLS_DLV_GROUP_MAX) {
		// the grouping kernel sees the first MI_CLS_DLV_GROUP_MAX entries only:
		// a larger burst must not ask for groups (its tail would be lost)
		for (uint32_t j = 0; j < a->n; ++j)
			if (a->dlv[j].qid != 0xFFu)
				return -E2BIG;
	}
	uint64_t t;
	int rc = ticket_begin(c, &t);
	if (rc)
		return rc;
	const unsigned grid = (a->n + 15u) / 16u + 1u;
	rc = mi_cls_launch_deliver(grid, c->dstream, *a);
	if (rc)
		return rc;
	return ticket_commit(c, t, c->dstream, ticket);
}

// The receive chain of one burst (mi_cls.h): its classification (zero copy:
// frames and descriptors in page-locked memory; the records into the ticket
// slot's HBM arrays), the decisions behind it, the delivery after them
// (which also copies the records out to args.res); one ticket.
extern "C" int mi_cls_rx_chain_submit(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes,
				      const mi_cls_rxc_args_t *a, uint64_t *ticket)
{
	if (!c || !a || !ticket || !c->loaded)
		return -EINVAL;
	*ticket = 0;
	if (a->n == 0)
		return 0;
	if (a->n > MI_CLS_DLV_GROUP_MAX || a->base != pkts || !mi_cls_host_mapped(pkts) ||
	    !mi_cls_host_mapped(a->soff) || !mi_cls_host_mapped(a->slen) || !mi_cls_host_mapped(a->res) ||
	    !mi_cls_host_mapped(a->tab) || !mi_cls_host_mapped(a->got) || !mi_cls_host_mapped(a->dec) ||
	    !mi_cls_host_mapped(a->ent) || !mi_cls_host_mapped(a->perm) || !mi_cls_host_mapped(a->gcnt) ||
	    !mi_cls_host_mapped(a->out) || ((uintptr_t)a->res & 15u) ||
	    (a->pk && (!mi_cls_host_mapped(a->pk) || !mi_cls_host_mapped(a->ppool))) ||
	    (a->stage && !a->pk))
		return -EINVAL;
	// the descriptors stay inside the batch (the stage kernel checks its own)
	if (!a->stage && !frames_padded_inside(a->soff, a->slen, a->n, bytes))
		return -EINVAL;
	uint64_t t;
	int rc = ticket_begin(c, &t);
	if (rc)
		return rc;
	// the whole chain on one of the context's two streams, by ticket
	// parity: a burst's kernels are ordered by their stream (no events
	// between them: each event record and stream wait costs the host 1.5-4
	// us), two bursts overlap, and one ticket event ends the chain.  (Two
	// further streams made for the chain ran it slower, 31 against 44
	// Mpkt/s on the pcap receive: profiles/r05rx_chain.txt.)
	hipStream_t xs = (t & 1u) ? c->dstream : c->stream;
	uint8_t *slot = c->d_rx + (t % 8) * RX_SLOT_BYTES;
	const mi_cls_rxdev_t d = { (mi_cls_result_t *)slot, (uint32_t *)(slot + RX_OFF_DEC),
				   (uint64_t *)(slot + RX_OFF_DQ), (uint16_t *)(slot + RX_OFF_LEN),
				   slot + RX_OFF_PP, (const mi_cls_rxtab_t *)(slot + RX_OFF_TAB),
				   a->stage ? 1u : 0u };
	// the slot's table copy, refreshed when the host table's stamp moved.
	// The copy reads a snapshot taken now, in the slot's own page-locked
	// buffer, not the caller's live table: the caller may rewrite that table
	// (a control-plane change) while this asynchronous copy is still queued,
	// and the burst must run on the table it was submitted with.  The slot's
	// previous chain, and so its copy, has completed (ticket_begin).
	if (c->tab_src[t % 8] != a->tab || c->tab_stamp[t % 8] != a->tab->stamp) {
		c->tab_src[t % 8] = nullptr;
		mi_cls_rxtab_t *snap = c->h_tab + (t % 8);
		memcpy(snap, a->tab, sizeof(mi_cls_rxtab_t));
		HIP_OK(hipMemcpyAsync(slot + RX_OFF_TAB, snap, sizeof(mi_cls_rxtab_t), hipMemcpyHostToDevice, xs));
		c->tab_src[t % 8] = a->tab;
		c->tab_stamp[t % 8] = snap->stamp;
	}
	rc = a->stage ? mi_cls_launch_rx_stage(xs, *a, d, bytes, false) : 0;
	if (rc)
		return rc;
	rc = mi_cls_classify(c, pkts, a->soff, a->slen, a->n, d.res, xs);
	if (rc)
		return rc;
	rc = mi_cls_launch_rx_chain(xs, *a, d, false);
	if (rc)
		return rc;
	return ticket_commit(c, t, xs, ticket);
}

extern "C" int mi_cls_classify_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return c ? host_wait(c, ticket) : -EINVAL;
}

// The features below answer a missing context with no_ctx()
static int feature_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return c ? host_wait(c, ticket) : no_ctx();
}

// ------------------------------------------------- pktout checksum insertion
// The context first, then the batch (an empty one is no error)
static int tx_check(const mi_cls_ctx_t *c, const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
		    const mi_cls_tx_desc_t *desc, uint32_t n)
{
	if (!c)
		return no_ctx();
	return n == 0 || (pkts && off && len && desc && ((uintptr_t)desc & 7u) == 0) ? 0 : -EINVAL;
}

extern "C" int mi_cls_chksum_insert(mi_cls_ctx_t *c, uint8_t *pkts, const uint32_t *off,
				    const uint16_t *len, const mi_cls_tx_desc_t *desc, uint32_t n,
				    uint64_t pktout_opt, uint8_t *done, void *stream)
{
	const int bad = tx_check(c, pkts, off, len, desc, n);
	if (bad || n == 0)
		return bad;
	HIP_OK(set_device(c->device));
	TxArgs a;
	a.pkts = pkts;
	a.off = off;
	a.len = len;
	a.desc = desc;
	a.done = done;
	a.n = n;
	a.opt = (uint32_t)pktout_opt;
	// one wave per 64-packet tile, persistent over the tiles: at most 6
	// blocks of TX_NW waves per CU (the kernel's registers admit 7 waves
	// per SIMD)
	const uint32_t tiles = (n + WAVE - 1) / WAVE;
	const uint32_t blocks = (tiles + TX_NW - 1) / TX_NW;
	const uint32_t max_grid = (uint32_t)c->num_cu * 6u;
	const int rc = mi_cls_launch_tx(blocks < max_grid ? blocks : max_grid, (hipStream_t)stream, a);
	if (rc)
		return rc;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int mi_cls_tx_hash(mi_cls_ctx_t *c, uint8_t *pkts, const uint32_t *off, const uint16_t *len,
			      const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t pktout_opt, uint8_t *done,
			      uint32_t hash_proto, uint32_t *hash_out, int chksum, void *stream);

// The flow hash asked for beside (ck) or instead of the checksums
// (mi_cls_tx_hash*); the checksum entries pass none
struct TxHashReq {
	uint32_t proto;
	uint32_t *out;
	int ck;
};

static int tx_launch(mi_cls_ctx_t *c, uint8_t *pkts, const uint32_t *off, const uint16_t *len,
		     const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t opt, uint8_t *done, const TxHashReq *hq,
		     uint32_t *hash, hipStream_t s)
{
	return hq ? mi_cls_tx_hash(c, pkts, off, len, desc, n, opt, done, hq->proto, hash, hq->ck, s)
		  : mi_cls_chksum_insert(c, pkts, off, len, desc, n, opt, done, s);
}

// A host batch on the context's stream, nothing waited for: in place when
// everything is page-locked (`done` and the hash words too, where given) and
// frames_padded_inside(bytes), else through the staging buffers (the frames
// copied back whole: only checksum fields differ; the hash alone writes none
// and copies none back).
static int tx_host_launch(mi_cls_ctx_t *c, uint8_t *pkts, size_t bytes, const uint32_t *off,
			  const uint16_t *len, const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t opt,
			  uint8_t *done, const TxHashReq *hq = nullptr)
{
	HIP_OK(set_device(c->device));
	uint8_t *zp = pkts, *zn = done;
	const uint32_t *zo = off;
	const uint16_t *zl = len;
	const mi_cls_tx_desc_t *zd = desc;
	uint32_t *zh = hq ? hq->out : nullptr;
	if (dev_views(zp, zo, zl, zd) && (!done || dev_views(zn)) && (!hq || dev_views(zh)) &&
	    frames_padded_inside(off, len, n, bytes))
		return tx_launch(c, zp, zo, zl, zd, n, opt, zn, hq, zh, c->stream);
	int rc = stage_up(c, pkts, bytes, bytes, off, len, n, n);
	if (rc)
		return rc;
	hipStream_t s = c->stream;
	mi_cls_tx_desc_t *d_desc = stg_tx_desc(c);
	uint32_t *d_hash = stg_txh_hash(c);
	uint8_t *d_done = hq ? stg_txh_done(c) : stg_tx_done(c);
	HIP_OK(hipMemcpyAsync(d_desc, desc, n * sizeof(mi_cls_tx_desc_t), hipMemcpyHostToDevice, s));
	rc = tx_launch(c, c->d_pk, c->d_off, c->d_len, d_desc, n, opt, done ? d_done : nullptr, hq, d_hash, s);
	if (rc)
		return rc;
	if (!hq || hq->ck)
		HIP_OK(hipMemcpyAsync(pkts, c->d_pk, bytes, hipMemcpyDeviceToHost, s));
	if (hq)
		HIP_OK(hipMemcpyAsync(hq->out, d_hash, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	if (done)
		HIP_OK(hipMemcpyAsync(done, d_done, n, hipMemcpyDeviceToHost, s));
	return 0;
}

// The checks of a host entry; hq: also its hash words and protocol bits
static bool tx_hash_req_ok(const TxHashReq *hq)
{
	return hq->out && ((uintptr_t)hq->out & 3u) == 0 && hq->proto != 0 && hq->proto < 64u;
}

static int tx_host_check(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes, const uint32_t *off,
			 const uint16_t *len, const mi_cls_tx_desc_t *desc, uint32_t n,
			 const TxHashReq *hq = nullptr)
{
	const int rc = tx_check(c, pkts, off, len, desc, n);
	return rc || n == 0 || (frames_inside(off, len, n, bytes) && (!hq || tx_hash_req_ok(hq))) ? rc : -EINVAL;
}

extern "C" int mi_cls_chksum_insert_host(mi_cls_ctx_t *c, uint8_t *pkts, size_t bytes,
					 const uint32_t *off, const uint16_t *len,
					 const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t opt,
					 uint8_t *done)
{
	const int rc = tx_host_check(c, pkts, bytes, off, len, desc, n);
	if (rc || n == 0)
		return rc;
	return host_run(c, nullptr, [&] { return tx_host_launch(c, pkts, bytes, off, len, desc, n, opt, done); });
}

extern "C" int mi_cls_chksum_insert_host_submit(mi_cls_ctx_t *c, uint8_t *pkts, size_t bytes,
						const uint32_t *off, const uint16_t *len,
						const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t opt,
						uint8_t *done, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = tx_host_check(c, pkts, bytes, off, len, desc, n);
	if (rc || n == 0)
		return rc;
	return host_run(c, ticket, [&] { return tx_host_launch(c, pkts, bytes, off, len, desc, n, opt, done); });
}

extern "C" int mi_cls_chksum_insert_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ------------------------------------------------------- the pktin flow hash
// (pktio/loop.c:479-530 get_dest_queue): the transmit kernel with the hash
// step, beside the checksums (chksum != 0) or alone
extern "C" int mi_cls_tx_hash(mi_cls_ctx_t *c, uint8_t *pkts, const uint32_t *off, const uint16_t *len,
			      const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t pktout_opt, uint8_t *done,
			      uint32_t hash_proto, uint32_t *hash_out, int chksum, void *stream)
{
	const TxHashReq hq = { hash_proto, hash_out, chksum };
	const int bad = tx_check(c, pkts, off, len, desc, n);
	if (bad || n == 0)
		return bad;
	if (!tx_hash_req_ok(&hq))
		return -EINVAL;
	HIP_OK(set_device(c->device));
	TxHashArgs a;
	a.pkts = pkts;
	a.off = off;
	a.len = len;
	a.desc = desc;
	a.done = done;
	a.n = n;
	a.opt = (uint32_t)pktout_opt;
	a.hash = hash_out;
	a.hash_proto = hash_proto;
	a.rsv = 0;
	// the grid of mi_cls_chksum_insert
	const uint32_t tiles = (n + WAVE - 1) / WAVE;
	const uint32_t blocks = (tiles + TX_NW - 1) / TX_NW;
	const uint32_t max_grid = (uint32_t)c->num_cu * 6u;
	const int rc = mi_cls_launch_tx_hash(chksum != 0, blocks < max_grid ? blocks : max_grid,
					     (hipStream_t)stream, a);
	if (rc)
		return rc;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// The host entries: tx_host_check / tx_host_launch with the hash request
extern "C" int mi_cls_tx_hash_host(mi_cls_ctx_t *c, uint8_t *pkts, size_t bytes, const uint32_t *off,
				   const uint16_t *len, const mi_cls_tx_desc_t *desc, uint32_t n, uint64_t opt,
				   uint8_t *done, uint32_t hash_proto, uint32_t *hash_out, int chksum)
{
	const TxHashReq hq = { hash_proto, hash_out, chksum };
	const int rc = tx_host_check(c, pkts, bytes, off, len, desc, n, &hq);
	if (rc || n == 0)
		return rc;
	return host_run(c, nullptr, [&] {
		return tx_host_launch(c, pkts, bytes, off, len, desc, n, opt, done, &hq);
	});
}

extern "C" int mi_cls_tx_hash_host_submit(mi_cls_ctx_t *c, uint8_t *pkts, size_t bytes, const uint32_t *off,
					  const uint16_t *len, const mi_cls_tx_desc_t *desc, uint32_t n,
					  uint64_t opt, uint8_t *done, uint32_t hash_proto, uint32_t *hash_out,
					  int chksum, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const TxHashReq hq = { hash_proto, hash_out, chksum };
	const int rc = tx_host_check(c, pkts, bytes, off, len, desc, n, &hq);
	if (rc || n == 0)
		return rc;
	return host_run(c, ticket, [&] {
		return tx_host_launch(c, pkts, bytes, off, len, desc, n, opt, done, &hq);
	});
}

extern "C" int mi_cls_tx_hash_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ------------------------------------------------------ the parse on its own
static int parse_check(const mi_cls_ctx_t *c, const mi_cls_parse_param_t *pp)
{
	// the parameters first: a bad one is -EINVAL with or without a device
	if (!pp || pp->proto < MI_CLS_PROTO_ETH || pp->proto > MI_CLS_PROTO_IPV6 ||
	    pp->last_layer < MI_CLS_LAYER_L2 || pp->last_layer > MI_CLS_LAYER_ALL)
		return -EINVAL;
	if (!c)
		return no_ctx();
	return 0;
}

extern "C" int mi_cls_parse(mi_cls_ctx_t *c, const uint8_t *pkts, const uint32_t *off,
			    const uint16_t *len, uint32_t n, const mi_cls_parse_param_t *pp,
			    mi_cls_result_t *out, void *stream)
{
	int rc = parse_check(c, pp);
	if (rc)
		return rc;
	if (n == 0)
		return 0;
	if (!pkts || !off || !len || !out || ((uintptr_t)out & 15u) != 0)
		return -EINVAL;
	HIP_OK(set_device(c->device));
	ParseArgs a;
	a.pkts = pkts;
	a.off = off;
	a.len = len;
	a.out = out;
	a.n = n;
	a.layer = pp->last_layer;
	// odp_proto_chksums_t bits 0-3 are the pktin option bits 2-5; what the
	// layer leaves of the selection: nothing at L2 (the return precedes
	// parse_ipv4), the IPv4 header checksum at L3
	uint32_t ck = (pp->chksums & 0xFu) << 2;
	if (pp->last_layer == MI_CLS_LAYER_L2)
		ck = 0;
	else if (pp->last_layer == MI_CLS_LAYER_L3)
		ck &= OPT_IPV4_CK;
	a.opt = ck;
	// one wave per 64-packet tile, persistent over the tiles: the blocks of
	// PRS_NW waves a CU holds at once, 4 (3 with the checksum code: its
	// registers and its 41 KB of LDS admit 3 waves per SIMD)
	const uint32_t tiles = (n + WAVE - 1) / WAVE;
	const uint32_t blocks = (tiles + PRS_NW - 1) / PRS_NW;
	const uint32_t max_grid = (uint32_t)c->num_cu * (ck ? 3u : 4u);
	const uint32_t grid = blocks < max_grid ? blocks : max_grid;
	uint32_t *last = c->last;
	last[0] = PRS_NW;
	last[1] = last[2] = last[3] = last[4] = 0;
	last[5] = ck != 0;
	last[6] = grid;
	rc = mi_cls_launch_parse(pp->proto, ck != 0, grid, (hipStream_t)stream, a);
	if (rc)
		return rc;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// A host batch on the context's stream, nothing waited for: in place when
// everything is page-locked, frames_padded_inside(bytes) and the records are
// 16-B aligned, else through the staging buffers (only the records come back).
static int parse_host_launch(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes, const uint32_t *off,
			     const uint16_t *len, uint32_t n, const mi_cls_parse_param_t *pp,
			     mi_cls_result_t *out)
{
	HIP_OK(set_device(c->device));
	const uint8_t *zp = pkts;
	const uint32_t *zo = off;
	const uint16_t *zl = len;
	mi_cls_result_t *zr = out;
	if (dev_views(zp, zo, zl, zr) && frames_padded_inside(off, len, n, bytes) && ((uintptr_t)zr & 15u) == 0)
		return mi_cls_parse(c, zp, zo, zl, n, pp, zr, c->stream);
	int rc = stage_up(c, pkts, bytes, bytes, off, len, n, n);
	if (rc)
		return rc;
	rc = mi_cls_parse(c, c->d_pk, c->d_off, c->d_len, n, pp, c->d_out, c->stream);
	if (rc)
		return rc;
	HIP_OK(hipMemcpyAsync(out, c->d_out, n * sizeof(mi_cls_result_t), hipMemcpyDeviceToHost, c->stream));
	return 0;
}

static int parse_host_check(const mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes, const uint32_t *off,
			    const uint16_t *len, uint32_t n, const mi_cls_parse_param_t *pp,
			    const mi_cls_result_t *out)
{
	const int rc = parse_check(c, pp);
	if (rc || n == 0)
		return rc;
	return pkts && off && len && out && frames_inside(off, len, n, bytes) ? 0 : -EINVAL;
}

extern "C" int mi_cls_parse_host(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes, const uint32_t *off,
				 const uint16_t *len, uint32_t n, const mi_cls_parse_param_t *pp,
				 mi_cls_result_t *out)
{
	const int rc = parse_host_check(c, pkts, bytes, off, len, n, pp, out);
	if (rc || n == 0)
		return rc;
	return host_run(c, nullptr, [&] { return parse_host_launch(c, pkts, bytes, off, len, n, pp, out); });
}

extern "C" int mi_cls_parse_host_submit(mi_cls_ctx_t *c, const uint8_t *pkts, size_t bytes,
					const uint32_t *off, const uint16_t *len, uint32_t n,
					const mi_cls_parse_param_t *pp, mi_cls_result_t *out,
					uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = parse_host_check(c, pkts, bytes, off, len, n, pp, out);
	if (rc || n == 0)
		return rc;
	return host_run(c, ticket, [&] { return parse_host_launch(c, pkts, bytes, off, len, n, pp, out); });
}

extern "C" int mi_cls_parse_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ----------------------------------------------------------- the enqueue plan
// The plan's scratch in the context, by the staging buffers' policy (grown by
// 1.5x, kept): per record the key (2 B), the first pass' order and high digits
// (4 + 1 B) and the staged form's perm (4 B); of fixed size the table's device
// copy, the count matrix, the counters and the staged form's gbeg and out.
#define ENQ_ALIGN(x) (((size_t)(x) + 255u) & ~(size_t)255u)
#define ENQ_FIX_TAB 0u
#define ENQ_FIX_MAT (ENQ_FIX_TAB + ENQ_ALIGN(sizeof(mi_cls_enq_tab_t)))
#define ENQ_FIX_CTR (ENQ_FIX_MAT + ENQ_ALIGN(((size_t)MI_CLS_ENQ_GRID << MI_CLS_ENQ_DIGIT) * 4u))
#define ENQ_FIX_OUT (ENQ_FIX_CTR + ENQ_ALIGN(sizeof(mi_cls_enq_out_t)))
#define ENQ_FIX_GBEG (ENQ_FIX_OUT + ENQ_ALIGN(sizeof(mi_cls_enq_out_t)))
#define ENQ_FIX_BYTES (ENQ_FIX_GBEG + ENQ_ALIGN(((size_t)MI_CLS_ENQ_DST_MAX + 2u) * 4u))

static uint16_t *enq_key16(const mi_cls_ctx_t *c) { return (uint16_t *)c->d_enq; }
static uint32_t *enq_tperm(const mi_cls_ctx_t *c) { return (uint32_t *)(c->d_enq + ENQ_ALIGN(2u * c->enq_cap)); }
static uint32_t *enq_sperm(const mi_cls_ctx_t *c) { return enq_tperm(c) + ENQ_ALIGN(c->enq_cap) ; }
static uint8_t *enq_hi8(const mi_cls_ctx_t *c) { return (uint8_t *)(enq_sperm(c) + ENQ_ALIGN(c->enq_cap)); }

// Scratch for n records.  Before it is replaced, and before the table's
// snapshot or device copy is rewritten, the previous plan has ended (enq_ev).
static int enq_idle(mi_cls_ctx_t *c)
{
	if (c->enq_used)
		HIP_OK(hipEventSynchronize(c->enq_ev));
	return 0;
}

static int enq_scratch(mi_cls_ctx_t *c, uint32_t n)
{
	if (!c->d_enq_fix) {
		if (hipEventCreateWithFlags(&c->enq_ev, hipEventDisableTiming) != hipSuccess)
			return -EIO;
		if (hipHostMalloc((void **)&c->h_enq_tab, sizeof(mi_cls_enq_tab_t), hipHostMallocDefault) != hipSuccess ||
		    hipMalloc((void **)&c->d_enq_fix, ENQ_FIX_BYTES) != hipSuccess)
			return -ENOMEM;
	}
	if (n > c->enq_cap) {
		const int rc = enq_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_enq);
		c->d_enq = nullptr;
		c->enq_cap = 0;
		const size_t cap = n < 4096u ? 4096u : (size_t)n + n / 2;
		if (hipMalloc((void **)&c->d_enq, ENQ_ALIGN(2u * cap) + 8u * ENQ_ALIGN(cap) + ENQ_ALIGN(cap)) != hipSuccess)
			return -ENOMEM;
		c->enq_cap = cap;
	}
	return 0;
}

// The context and the table first, then the batch
static int enq_check(const mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
		     const mi_cls_enq_tab_t *tab, const uint32_t *perm, const uint32_t *gbeg,
		     const mi_cls_enq_out_t *out)
{
	if (!tab)
		return -EINVAL;
	if (tab->ndst > MI_CLS_ENQ_DST_MAX)
		return -E2BIG;
	if (!c)
		return no_ctx();
	if (!gbeg || !out || ((uintptr_t)out & 7u) != 0)
		return -EINVAL;
	return n == 0 || (res && len && perm) ? 0 : -EINVAL;
}

extern "C" int mi_cls_enq_plan(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
			       const mi_cls_enq_tab_t *tab, uint32_t *perm, uint32_t *gbeg,
			       mi_cls_enq_out_t *out, void *stream)
{
	int rc = enq_check(c, res, len, n, tab, perm, gbeg, out);
	if (rc)
		return rc;
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(set_device(c->device));
	rc = enq_scratch(c, n);
	if (rc)
		return rc;
	// the scratch is one plan's at a time: a plan on another stream follows
	// the previous one
	if (c->enq_used && c->enq_last != st)
		HIP_OK(hipStreamWaitEvent(st, c->enq_ev, 0));
	// the table's device copy, refreshed when the host table's stamp moved
	mi_cls_enq_tab_t *dtab = (mi_cls_enq_tab_t *)(c->d_enq_fix + ENQ_FIX_TAB);
	if (!c->enq_tab_src || c->enq_tab_src != tab || c->enq_tab_stamp != tab->stamp) {
		rc = enq_idle(c);
		if (rc)
			return rc;
		memcpy(c->h_enq_tab, tab, sizeof(*tab));
		c->enq_tab_src = nullptr;
		HIP_OK(hipMemcpyAsync(dtab, c->h_enq_tab, sizeof(*tab), hipMemcpyHostToDevice, st));
		c->enq_tab_src = tab;
		c->enq_tab_stamp = c->h_enq_tab->stamp;
	}
	EnqArgs a;
	memset(&a, 0, sizeof(a));
	a.res = res;
	a.len = len;
	a.tab = dtab;
	a.n = n;
	a.ndst = tab->ndst;
	const uint64_t tiles = ((uint64_t)n + MI_CLS_ENQ_TILE - 1u) / MI_CLS_ENQ_TILE;
	a.grid = (uint32_t)(tiles < MI_CLS_ENQ_GRID ? tiles : MI_CLS_ENQ_GRID);
	a.tpb = a.grid ? (uint32_t)((tiles + a.grid - 1u) / a.grid) : 0u;
	a.key16 = enq_key16(c);
	a.hi8 = enq_hi8(c);
	a.tperm = enq_tperm(c);
	a.mat = (uint32_t *)(c->d_enq_fix + ENQ_FIX_MAT);
	a.ctr = (unsigned long long *)(c->d_enq_fix + ENQ_FIX_CTR);
	a.perm = perm;
	a.gbeg = gbeg;
	a.out = out;
	// keys 0 .. ndst: one stable pass when they have one digit
	const int passes = n == 0 ? 0 : a.ndst + 1u <= (1u << MI_CLS_ENQ_DIGIT) ? 1 : 2;
	a.passes = (uint32_t)passes;
	// this call's counters start from zero, whatever the last one left
	HIP_OK(hipMemsetAsync(a.ctr, 0, sizeof(mi_cls_enq_out_t), st));
	uint32_t *last = c->last;
	last[0] = 128u + MI_CLS_ENQ_TILE / WAVE;
	last[1] = (uint32_t)passes;
	last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = a.grid;
	rc = mi_cls_launch_enq(st, a, passes, false);
	if (rc)
		return rc;
	HIP_OK(hipEventRecord(c->enq_ev, st));
	c->enq_used = true;
	c->enq_last = st;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// A host batch on the context's stream, nothing waited for: in place when
// every array is page-locked, else the records and lengths through the
// staging buffers and perm, gbeg and out through the scratch.
static int enq_host_launch(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
			   const mi_cls_enq_tab_t *tab, uint32_t *perm, uint32_t *gbeg, mi_cls_enq_out_t *out)
{
	HIP_OK(set_device(c->device));
	const mi_cls_result_t *zr = res;
	const uint16_t *zl = len;
	uint32_t *zp = perm, *zg = gbeg;
	mi_cls_enq_out_t *zo = out;
	if (dev_views(zr, zl, zp, zg, zo))
		return mi_cls_enq_plan(c, zr, zl, n, tab, zp, zg, zo, c->stream);
	int rc = stage_bufs(c, 0, n);
	if (!rc)
		rc = enq_scratch(c, n);
	if (rc)
		return rc;
	if (n) {
		HIP_OK(hipMemcpyAsync(c->d_out, res, n * sizeof(mi_cls_result_t), hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(c->d_len, len, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
	}
	uint32_t *dg = (uint32_t *)(c->d_enq_fix + ENQ_FIX_GBEG);
	mi_cls_enq_out_t *dout = (mi_cls_enq_out_t *)(c->d_enq_fix + ENQ_FIX_OUT);
	rc = mi_cls_enq_plan(c, c->d_out, c->d_len, n, tab, enq_sperm(c), dg, dout, c->stream);
	if (rc)
		return rc;
	if (n)
		HIP_OK(hipMemcpyAsync(perm, enq_sperm(c), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_OK(hipMemcpyAsync(gbeg, dg, ((size_t)tab->ndst + 2u) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_OK(hipMemcpyAsync(out, dout, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
	// the scratch is this plan's until the copies have read it
	HIP_OK(hipEventRecord(c->enq_ev, c->stream));
	return 0;
}

extern "C" int mi_cls_enq_plan_host(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
				    uint32_t n, const mi_cls_enq_tab_t *tab, uint32_t *perm, uint32_t *gbeg,
				    mi_cls_enq_out_t *out)
{
	const int rc = enq_check(c, res, len, n, tab, perm, gbeg, out);
	if (rc)
		return rc;
	return host_run(c, nullptr, [&] { return enq_host_launch(c, res, len, n, tab, perm, gbeg, out); });
}

extern "C" int mi_cls_enq_plan_host_submit(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
					   uint32_t n, const mi_cls_enq_tab_t *tab, uint32_t *perm,
					   uint32_t *gbeg, mi_cls_enq_out_t *out, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = enq_check(c, res, len, n, tab, perm, gbeg, out);
	if (rc)
		return rc;
	return host_run(c, ticket, [&] { return enq_host_launch(c, res, len, n, tab, perm, gbeg, out); });
}

extern "C" int mi_cls_enq_plan_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// --------------------------------------------------------------- the run plan
// The run plan's scratch in the context, by the enqueue plan's policy: per
// record the key (4 B) and a run's head (8 B); of fixed size the two tables'
// device copies, the blocks' summaries and what the scan makes of them, the
// totals, the counters and the staged form's out.  The staged form's seq and
// runs have a buffer of their own (4 B per record + 16 B per run of run_cap).
#define RUN_FIX_TAB 0u
#define RUN_FIX_RTAB (RUN_FIX_TAB + ENQ_ALIGN(sizeof(mi_cls_enq_tab_t)))
#define RUN_FIX_SUM (RUN_FIX_RTAB + ENQ_ALIGN(sizeof(mi_cls_run_tab_t)))
#define RUN_FIX_PRE (RUN_FIX_SUM + ENQ_ALIGN((size_t)MI_CLS_RUN_GRID * 8u * 4u))
#define RUN_FIX_TOT (RUN_FIX_PRE + ENQ_ALIGN((size_t)MI_CLS_RUN_GRID * 16u))
#define RUN_FIX_CTR (RUN_FIX_TOT + ENQ_ALIGN(8u))
#define RUN_FIX_OUT (RUN_FIX_CTR + ENQ_ALIGN(sizeof(mi_cls_run_out_t)))
#define RUN_FIX_BYTES (RUN_FIX_OUT + ENQ_ALIGN(sizeof(mi_cls_run_out_t)))

static uint2 *run_head(const mi_cls_ctx_t *c) { return (uint2 *)c->d_run; }
static uint32_t *run_key(const mi_cls_ctx_t *c) { return (uint32_t *)(c->d_run + ENQ_ALIGN(8u * c->run_cap)); }

// Before the scratch is replaced, and before a table's snapshot or device copy
// is rewritten, the previous run plan has ended (run_ev).
static int run_idle(mi_cls_ctx_t *c)
{
	if (c->run_used)
		HIP_OK(hipEventSynchronize(c->run_ev));
	return 0;
}

static int run_scratch(mi_cls_ctx_t *c, uint32_t n, size_t staged)
{
	if (!c->d_run_fix) {
		if (!c->run_ev && hipEventCreateWithFlags(&c->run_ev, hipEventDisableTiming) != hipSuccess)
			return -EIO;
		if ((!c->h_run_tab &&
		     hipHostMalloc((void **)&c->h_run_tab, ENQ_ALIGN(sizeof(mi_cls_enq_tab_t)) + sizeof(mi_cls_run_tab_t),
				   hipHostMallocDefault) != hipSuccess) ||
		    hipMalloc((void **)&c->d_run_fix, RUN_FIX_BYTES) != hipSuccess)
			return -ENOMEM;
	}
	if (n > c->run_cap) {
		const int rc = run_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_run);
		c->d_run = nullptr;
		c->run_cap = 0;
		const size_t cap = n < 4096u ? 4096u : (size_t)n + n / 2;
		if (hipMalloc((void **)&c->d_run, ENQ_ALIGN(8u * cap) + ENQ_ALIGN(4u * cap)) != hipSuccess)
			return -ENOMEM;
		c->run_cap = cap;
	}
	if (staged > c->run_st_cap) {
		const int rc = run_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_run_st);
		c->d_run_st = nullptr;
		c->run_st_cap = 0;
		const size_t cap = staged < 65536u ? 65536u : staged + staged / 2;
		if (hipMalloc((void **)&c->d_run_st, cap) != hipSuccess)
			return -ENOMEM;
		c->run_st_cap = cap;
	}
	return 0;
}

// The tables first (host memory, no device needed), then the context, then
// the batch
static int run_check(const mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
		     const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab, const uint32_t *seq,
		     const mi_cls_run_t *runs, uint32_t run_cap, const mi_cls_run_out_t *out)
{
	if (!tab || !rtab)
		return -EINVAL;
	if (tab->ndst > MI_CLS_ENQ_DST_MAX)
		return -E2BIG;
	for (uint32_t i = 0; i < 256u; ++i)
		if ((rtab->mode[i] & MI_CLS_RUN_VEC) && (rtab->vmax[i] == 0 || rtab->vslot[i] >= MI_CLS_RUN_VSLOTS))
			return -EINVAL;
	if (!c)
		return no_ctx();
	if (!out || ((uintptr_t)out & 7u) != 0)
		return -EINVAL;
	if (n == 0)
		return 0;
	return res && len && seq && (run_cap == 0 || (runs && ((uintptr_t)runs & 15u) == 0)) ? 0 : -EINVAL;
}

// One table's device copy, refreshed when the host table's stamp moved
static int run_tab_sync(mi_cls_ctx_t *c, int which, const void *tab, uint64_t stamp, size_t bytes, void *snap,
			void *dtab, hipStream_t st)
{
	if (c->run_tab_src[which] && c->run_tab_src[which] == tab && c->run_tab_stamp[which] == stamp)
		return 0;
	const int rc = run_idle(c);
	if (rc)
		return rc;
	memcpy(snap, tab, bytes);
	c->run_tab_src[which] = nullptr;
	HIP_OK(hipMemcpyAsync(dtab, snap, bytes, hipMemcpyHostToDevice, st));
	c->run_tab_src[which] = tab;
	c->run_tab_stamp[which] = stamp;
	return 0;
}

extern "C" int mi_cls_enq_runs(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
			       const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab, uint32_t burst,
			       uint32_t *seq, mi_cls_run_t *runs, uint32_t run_cap, mi_cls_run_out_t *out,
			       void *stream)
{
	int rc = run_check(c, res, len, n, tab, rtab, seq, runs, run_cap, out);
	if (rc)
		return rc;
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(set_device(c->device));
	rc = run_scratch(c, n, 0);
	if (rc)
		return rc;
	// the scratch is one plan's at a time: a plan on another stream follows
	// the previous one
	if (c->run_used && c->run_last != st)
		HIP_OK(hipStreamWaitEvent(st, c->run_ev, 0));
	mi_cls_enq_tab_t *dtab = (mi_cls_enq_tab_t *)(c->d_run_fix + RUN_FIX_TAB);
	mi_cls_run_tab_t *drtab = (mi_cls_run_tab_t *)(c->d_run_fix + RUN_FIX_RTAB);
	const uint32_t ndst = tab->ndst;
	rc = run_tab_sync(c, 0, tab, tab->stamp, sizeof(*tab), c->h_run_tab, dtab, st);
	if (!rc)
		rc = run_tab_sync(c, 1, rtab, rtab->stamp, sizeof(*rtab),
				  c->h_run_tab + ENQ_ALIGN(sizeof(mi_cls_enq_tab_t)), drtab, st);
	if (rc)
		return rc;
	RunArgs a;
	memset(&a, 0, sizeof(a));
	a.res = res;
	a.len = len;
	a.tab = dtab;
	a.rtab = drtab;
	a.n = n;
	a.ndst = ndst;
	const uint64_t tiles = ((uint64_t)n + MI_CLS_RUN_TILE - 1u) / MI_CLS_RUN_TILE;
	a.grid = (uint32_t)(tiles < MI_CLS_RUN_GRID ? tiles : MI_CLS_RUN_GRID);
	a.tpb = a.grid ? (uint32_t)((tiles + a.grid - 1u) / a.grid) : 0u;
	a.burst = burst ? burst : 0xFFFFFFFFu;   // i / burst == 0 for every i < n
	a.run_cap = run_cap;
	a.key = run_key(c);
	a.head = run_head(c);
	a.sum = (uint32_t *)(c->d_run_fix + RUN_FIX_SUM);
	a.pre = (uint4 *)(c->d_run_fix + RUN_FIX_PRE);
	a.tot = (uint32_t *)(c->d_run_fix + RUN_FIX_TOT);
	a.ctr = (unsigned long long *)(c->d_run_fix + RUN_FIX_CTR);
	a.seq = seq;
	a.runs = runs;
	a.out = out;
	// this call's counters start from zero, whatever the last one left
	HIP_OK(hipMemsetAsync(a.ctr, 0, sizeof(mi_cls_run_out_t), st));
	uint32_t *last = c->last;
	last[0] = 192u + MI_CLS_RUN_TILE / WAVE;
	last[1] = n ? 5u : 1u;
	last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = a.grid;
	rc = mi_cls_launch_run(st, a, false);
	if (rc)
		return rc;
	HIP_OK(hipEventRecord(c->run_ev, st));
	c->run_used = true;
	c->run_last = st;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// A host batch on the context's stream, nothing waited for: in place when
// every array is page-locked, else the records and lengths through the
// staging buffers and seq, runs and out through the scratch.  The staged
// runs go up before they come back: the entries past nruns, which the device
// alone knows, keep the caller's values.
static int run_host_launch(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
			   const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab, uint32_t burst,
			   uint32_t *seq, mi_cls_run_t *runs, uint32_t run_cap, mi_cls_run_out_t *out)
{
	HIP_OK(set_device(c->device));
	if (n == 0)
		run_cap = 0;   // no run is written
	const mi_cls_result_t *zr = res;
	const uint16_t *zl = len;
	uint32_t *zs = seq;
	mi_cls_run_t *zu = runs;
	mi_cls_run_out_t *zo = out;
	if (dev_views(zo) && (n == 0 || (dev_views(zr, zl, zs) && (run_cap == 0 || dev_views(zu)))))
		return mi_cls_enq_runs(c, zr, zl, n, tab, rtab, burst, zs, zu, run_cap, zo, c->stream);
	const size_t seq_bytes = ENQ_ALIGN((size_t)n * sizeof(uint32_t));
	const size_t runs_bytes = (size_t)run_cap * sizeof(mi_cls_run_t);
	int rc = stage_bufs(c, 0, n);
	if (!rc)
		rc = run_scratch(c, n, seq_bytes + runs_bytes);
	if (rc)
		return rc;
	uint32_t *dseq = (uint32_t *)c->d_run_st;
	mi_cls_run_t *druns = (mi_cls_run_t *)(c->d_run_st + seq_bytes);
	mi_cls_run_out_t *dout = (mi_cls_run_out_t *)(c->d_run_fix + RUN_FIX_OUT);
	if (n) {
		HIP_OK(hipMemcpyAsync(c->d_out, res, n * sizeof(mi_cls_result_t), hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(c->d_len, len, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
	}
	if (runs_bytes)
		HIP_OK(hipMemcpyAsync(druns, runs, runs_bytes, hipMemcpyHostToDevice, c->stream));
	rc = mi_cls_enq_runs(c, c->d_out, c->d_len, n, tab, rtab, burst, dseq, druns, run_cap, dout, c->stream);
	if (rc)
		return rc;
	if (n)
		HIP_OK(hipMemcpyAsync(seq, dseq, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	if (runs_bytes)
		HIP_OK(hipMemcpyAsync(runs, druns, runs_bytes, hipMemcpyDeviceToHost, c->stream));
	HIP_OK(hipMemcpyAsync(out, dout, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
	// the scratch is this plan's until the copies have read it
	HIP_OK(hipEventRecord(c->run_ev, c->stream));
	return 0;
}

extern "C" int mi_cls_enq_runs_host(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
				    uint32_t n, const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab,
				    uint32_t burst, uint32_t *seq, mi_cls_run_t *runs, uint32_t run_cap,
				    mi_cls_run_out_t *out)
{
	const int rc = run_check(c, res, len, n, tab, rtab, seq, runs, run_cap, out);
	if (rc)
		return rc;
	return host_run(c, nullptr,
			[&] { return run_host_launch(c, res, len, n, tab, rtab, burst, seq, runs, run_cap, out); });
}

extern "C" int mi_cls_enq_runs_host_submit(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
					   uint32_t n, const mi_cls_enq_tab_t *tab, const mi_cls_run_tab_t *rtab,
					   uint32_t burst, uint32_t *seq, mi_cls_run_t *runs, uint32_t run_cap,
					   mi_cls_run_out_t *out, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = run_check(c, res, len, n, tab, rtab, seq, runs, run_cap, out);
	if (rc)
		return rc;
	return host_run(c, ticket,
			[&] { return run_host_launch(c, res, len, n, tab, rtab, burst, seq, runs, run_cap, out); });
}

extern "C" int mi_cls_enq_runs_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// -------------------------------------------------------------- the pool plan
// The pool plan's scratch in the context, by the enqueue plan's policy.  Of
// fixed size: the table's device copy, the count matrix (slot-major), the two
// counters and the staged form's out.  The device path needs nothing per
// record; the staged host form keeps own (1 B), dec and idx (4 B each) per
// record in a buffer of its own, and its res_out in the staged records' place.
#define POOL_FIX_TAB 0u
#define POOL_FIX_CNT (POOL_FIX_TAB + ENQ_ALIGN(sizeof(mi_cls_pool_tab_t)))
#define POOL_FIX_CTR (POOL_FIX_CNT + ENQ_ALIGN((size_t)MI_CLS_POOL_SLOTS * MI_CLS_POOL_GRID * 4u))
#define POOL_FIX_OUT (POOL_FIX_CTR + ENQ_ALIGN(16u))
#define POOL_FIX_BYTES (POOL_FIX_OUT + ENQ_ALIGN(sizeof(mi_cls_pool_out_t)))

static uint32_t *pool_st_dec(const mi_cls_ctx_t *c) { return (uint32_t *)c->d_pool_st; }
static uint32_t *pool_st_idx(const mi_cls_ctx_t *c) { return (uint32_t *)(c->d_pool_st + ENQ_ALIGN(4u * c->pool_st_cap)); }
static uint8_t *pool_st_own(const mi_cls_ctx_t *c) { return c->d_pool_st + 2u * ENQ_ALIGN(4u * c->pool_st_cap); }

// Before the scratch is replaced, and before the table's snapshot or device
// copy is rewritten, the previous pool plan has ended (pool_ev).
static int pool_idle(mi_cls_ctx_t *c)
{
	if (c->pool_used)
		HIP_OK(hipEventSynchronize(c->pool_ev));
	return 0;
}

// staged: records of the staged host form (0: the device path)
static int pool_scratch(mi_cls_ctx_t *c, uint32_t staged)
{
	if (!c->d_pool_fix) {
		if (!c->pool_ev && hipEventCreateWithFlags(&c->pool_ev, hipEventDisableTiming) != hipSuccess)
			return -EIO;
		if ((!c->h_pool_tab &&
		     hipHostMalloc((void **)&c->h_pool_tab, sizeof(mi_cls_pool_tab_t), hipHostMallocDefault) != hipSuccess) ||
		    hipMalloc((void **)&c->d_pool_fix, POOL_FIX_BYTES) != hipSuccess)
			return -ENOMEM;
	}
	if (staged > c->pool_st_cap) {
		const int rc = pool_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_pool_st);
		c->d_pool_st = nullptr;
		c->pool_st_cap = 0;
		const size_t cap = staged < 4096u ? 4096u : (size_t)staged + staged / 2;
		if (hipMalloc((void **)&c->d_pool_st, 2u * ENQ_ALIGN(4u * cap) + ENQ_ALIGN(cap)) != hipSuccess)
			return -ENOMEM;
		c->pool_st_cap = cap;
	}
	return 0;
}

// The table and the packets first (host memory, no device needed), then the
// context, then the batch
static int pool_check(const mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, uint32_t n,
		      const mi_cls_pool_tab_t *tab, const uint32_t *have, const uint32_t *base,
		      const mi_cls_result_t *res_out, const uint32_t *dec, const uint32_t *idx,
		      const mi_cls_pool_out_t *out)
{
	if (!tab || !have || !base || tab->nslot > MI_CLS_POOL_SLOTS || n > MI_CLS_MAX_BATCH)
		return -EINVAL;
	// an index stays below 0xFFFFFFFF, the value of "no packet"
	for (uint32_t k = 0; k < tab->nslot; ++k)
		if ((uint64_t)base[k] + (have[k] < n ? have[k] : n) > 0xFFFFFFFEull)
			return -EINVAL;
	if (!c)
		return no_ctx();
	if (!out || ((uintptr_t)out & 7u) != 0)
		return -EINVAL;
	if (n == 0)
		return 0;
	return res && len && res_out && dec && idx && (((uintptr_t)res | (uintptr_t)res_out) & 15u) == 0 ? 0 : -EINVAL;
}

extern "C" int mi_cls_pool_plan(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
				const uint8_t *own, uint32_t n, const mi_cls_pool_tab_t *tab,
				const uint32_t *have, const uint32_t *base, mi_cls_result_t *res_out, uint32_t *dec,
				uint32_t *idx, mi_cls_pool_out_t *out, void *stream)
{
	int rc = pool_check(c, res, len, n, tab, have, base, res_out, dec, idx, out);
	if (rc)
		return rc;
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(set_device(c->device));
	rc = pool_scratch(c, 0);
	if (rc)
		return rc;
	// the scratch is one plan's at a time: a plan on another stream follows
	// the previous one
	if (c->pool_used && c->pool_last != st)
		HIP_OK(hipStreamWaitEvent(st, c->pool_ev, 0));
	// the table's device copy, refreshed when the host table's stamp moved
	mi_cls_pool_tab_t *dtab = (mi_cls_pool_tab_t *)(c->d_pool_fix + POOL_FIX_TAB);
	const uint32_t nslot = tab->nslot;
	if (!c->pool_tab_src || c->pool_tab_src != tab || c->pool_tab_stamp != tab->stamp) {
		rc = pool_idle(c);
		if (rc)
			return rc;
		memcpy(c->h_pool_tab, tab, sizeof(*tab));
		c->pool_tab_src = nullptr;
		HIP_OK(hipMemcpyAsync(dtab, c->h_pool_tab, sizeof(*tab), hipMemcpyHostToDevice, st));
		c->pool_tab_src = tab;
		c->pool_tab_stamp = c->h_pool_tab->stamp;
	}
	PoolArgs a;
	memset(&a, 0, sizeof(a));
	a.res = res;
	a.len = len;
	a.own = own;
	a.tab = dtab;
	a.n = n;
	a.nslot = nslot;
	const uint64_t tiles = ((uint64_t)n + MI_CLS_POOL_TILE - 1u) / MI_CLS_POOL_TILE;
	a.grid = (uint32_t)(tiles < MI_CLS_POOL_GRID ? tiles : MI_CLS_POOL_GRID);
	a.tpb = a.grid ? (uint32_t)((tiles + a.grid - 1u) / a.grid) : 0u;
	for (uint32_t k = 0; k < MI_CLS_POOL_SLOTS; ++k) {
		a.have[k] = k < nslot ? have[k] : 0u;
		a.base[k] = k < nslot ? base[k] : 0u;
	}
	a.cnt = (uint32_t *)(c->d_pool_fix + POOL_FIX_CNT);
	a.ctr = (unsigned long long *)(c->d_pool_fix + POOL_FIX_CTR);
	a.res_out = res_out;
	a.dec = dec;
	a.idx = idx;
	a.out = out;
	// this call's counters start from zero, whatever the last one left
	HIP_OK(hipMemsetAsync(a.ctr, 0, 16u, st));
	uint32_t *last = c->last;
	last[0] = 256u + MI_CLS_POOL_TILE / WAVE;
	last[1] = n ? 3u : 1u;
	last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = a.grid;
	rc = mi_cls_launch_pool(st, a, false);
	if (rc)
		return rc;
	HIP_OK(hipEventRecord(c->pool_ev, st));
	c->pool_used = true;
	c->pool_last = st;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// A host batch on the context's stream, nothing waited for: in place when
// every array is page-locked, else the records and lengths through the
// staging buffers (res_out takes the staged records' place), own, dec and idx
// through the plan's staging buffer and out through the scratch.
static int pool_host_launch(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len, const uint8_t *own,
			    uint32_t n, const mi_cls_pool_tab_t *tab, const uint32_t *have, const uint32_t *base,
			    mi_cls_result_t *res_out, uint32_t *dec, uint32_t *idx, mi_cls_pool_out_t *out)
{
	HIP_OK(set_device(c->device));
	const mi_cls_result_t *zr = res;
	const uint16_t *zl = len;
	const uint8_t *zw = own;
	mi_cls_result_t *zq = res_out;
	uint32_t *zd = dec, *zi = idx;
	mi_cls_pool_out_t *zo = out;
	if (dev_views(zo) && (n == 0 || (dev_views(zr, zl, zq, zd, zi) && (!own || dev_views(zw)))))
		return mi_cls_pool_plan(c, zr, zl, n ? zw : nullptr, n, tab, have, base, zq, zd, zi, zo, c->stream);
	int rc = stage_bufs(c, 0, n);
	if (!rc)
		rc = pool_scratch(c, n ? n : 1u);
	if (rc)
		return rc;
	uint8_t *down = own && n ? pool_st_own(c) : nullptr;
	mi_cls_pool_out_t *dout = (mi_cls_pool_out_t *)(c->d_pool_fix + POOL_FIX_OUT);
	if (n) {
		HIP_OK(hipMemcpyAsync(c->d_out, res, n * sizeof(mi_cls_result_t), hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(c->d_len, len, n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
		if (down)
			HIP_OK(hipMemcpyAsync(down, own, n, hipMemcpyHostToDevice, c->stream));
	}
	rc = mi_cls_pool_plan(c, c->d_out, c->d_len, down, n, tab, have, base, c->d_out, pool_st_dec(c),
			      pool_st_idx(c), dout, c->stream);
	if (rc)
		return rc;
	if (n) {
		HIP_OK(hipMemcpyAsync(res_out, c->d_out, n * sizeof(mi_cls_result_t), hipMemcpyDeviceToHost, c->stream));
		HIP_OK(hipMemcpyAsync(dec, pool_st_dec(c), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		HIP_OK(hipMemcpyAsync(idx, pool_st_idx(c), n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	}
	HIP_OK(hipMemcpyAsync(out, dout, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
	// the scratch is this plan's until the copies have read it
	HIP_OK(hipEventRecord(c->pool_ev, c->stream));
	return 0;
}

extern "C" int mi_cls_pool_plan_host(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
				     const uint8_t *own, uint32_t n, const mi_cls_pool_tab_t *tab,
				     const uint32_t *have, const uint32_t *base, mi_cls_result_t *res_out,
				     uint32_t *dec, uint32_t *idx, mi_cls_pool_out_t *out)
{
	const int rc = pool_check(c, res, len, n, tab, have, base, res_out, dec, idx, out);
	if (rc)
		return rc;
	return host_run(c, nullptr,
			[&] { return pool_host_launch(c, res, len, own, n, tab, have, base, res_out, dec, idx, out); });
}

extern "C" int mi_cls_pool_plan_host_submit(mi_cls_ctx_t *c, const mi_cls_result_t *res, const uint16_t *len,
					    const uint8_t *own, uint32_t n, const mi_cls_pool_tab_t *tab,
					    const uint32_t *have, const uint32_t *base, mi_cls_result_t *res_out,
					    uint32_t *dec, uint32_t *idx, mi_cls_pool_out_t *out, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = pool_check(c, res, len, n, tab, have, base, res_out, dec, idx, out);
	if (rc)
		return rc;
	return host_run(c, ticket,
			[&] { return pool_host_launch(c, res, len, own, n, tab, have, base, res_out, dec, idx, out); });
}

extern "C" int mi_cls_pool_plan_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// -------------------------------------------------------------- the pool move
// The pool move's scratch in the context, by the pool plan's policy.  Of fixed
// size: the table's device copy with dst_queue behind it, the four counters
// and the staged form's out.  The device path needs nothing per entry; the
// staged host form keeps dec, idx (4 B each), pk and ent (8 B each) per record
// and got (8 B per packet) in a buffer of its own, of move_st_cap entries each.
#define MOVE_FIX_TAB 0u
#define MOVE_FIX_DSTQ (MOVE_FIX_TAB + ENQ_ALIGN(sizeof(mi_cls_enq_tab_t)))
#define MOVE_FIX_CTR (MOVE_FIX_DSTQ + ENQ_ALIGN((size_t)MI_CLS_ENQ_DST_MAX * 8u))
#define MOVE_FIX_OUT (MOVE_FIX_CTR + ENQ_ALIGN(sizeof(mi_cls_move_out_t)))
#define MOVE_FIX_BYTES (MOVE_FIX_OUT + ENQ_ALIGN(sizeof(mi_cls_move_out_t)))

static uint64_t *move_st_ent(const mi_cls_ctx_t *c) { return (uint64_t *)c->d_move_st; }
static uint64_t *move_st_pk(const mi_cls_ctx_t *c) { return (uint64_t *)(c->d_move_st + ENQ_ALIGN(8u * c->move_st_cap)); }
static uint64_t *move_st_got(const mi_cls_ctx_t *c) { return (uint64_t *)(c->d_move_st + 2u * ENQ_ALIGN(8u * c->move_st_cap)); }
static uint32_t *move_st_dec(const mi_cls_ctx_t *c) { return (uint32_t *)(c->d_move_st + 3u * ENQ_ALIGN(8u * c->move_st_cap)); }
static uint32_t *move_st_idx(const mi_cls_ctx_t *c) { return move_st_dec(c) + ENQ_ALIGN(4u * c->move_st_cap) / 4u; }

// Before the scratch is replaced, and before the table's snapshot or device
// copy is rewritten, the previous move has ended (move_ev).
static int move_idle(mi_cls_ctx_t *c)
{
	if (c->move_used)
		HIP_OK(hipEventSynchronize(c->move_ev));
	return 0;
}

// staged: entries of the staged host form (0: the device path)
static int move_scratch(mi_cls_ctx_t *c, uint32_t staged)
{
	if (!c->d_move_fix) {
		if (!c->move_ev && hipEventCreateWithFlags(&c->move_ev, hipEventDisableTiming) != hipSuccess)
			return -EIO;
		if ((!c->h_move_tab &&
		     hipHostMalloc((void **)&c->h_move_tab, MOVE_FIX_CTR, hipHostMallocDefault) != hipSuccess) ||
		    hipMalloc((void **)&c->d_move_fix, MOVE_FIX_BYTES) != hipSuccess)
			return -ENOMEM;
	}
	if (staged > c->move_st_cap) {
		const int rc = move_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_move_st);
		c->d_move_st = nullptr;
		c->move_st_cap = 0;
		const size_t cap = staged < 4096u ? 4096u : (size_t)staged + staged / 2;
		if (hipMalloc((void **)&c->d_move_st, 3u * ENQ_ALIGN(8u * cap) + 2u * ENQ_ALIGN(4u * cap)) != hipSuccess)
			return -ENOMEM;
		c->move_st_cap = cap;
	}
	return 0;
}

// The table and the scalars first (host memory, no device needed), then the
// context, then the batch
static int move_check(const mi_cls_ctx_t *c, const mi_cls_move_args_t *a)
{
	if (!a || !a->tab || a->n > MI_CLS_MAX_BATCH || a->pkts_bytes > 0xFFFFFFFFull || a->data_from_meta < 64u ||
	    (a->data_from_meta & 15u) != 0 || a->arena_lo + a->arena_bytes < a->arena_lo)
		return -EINVAL;
	if (a->tab->ndst > MI_CLS_ENQ_DST_MAX)
		return -E2BIG;
	if ((a->tab->ndst && !a->dst_queue) || (a->ngot && !a->got))
		return -EINVAL;
	if (!c)
		return no_ctx();
	if (!a->out || ((uintptr_t)a->out & 7u) != 0)
		return -EINVAL;
	if (a->n == 0)
		return 0;
	return a->pkts && a->off && a->len && a->res && a->dec && a->idx && a->ent && ((uintptr_t)a->res & 15u) == 0 &&
			       (((uintptr_t)a->ent | (uintptr_t)a->got | (uintptr_t)a->pk) & 7u) == 0 ? 0 : -EINVAL;
}

extern "C" int mi_cls_pool_move(mi_cls_ctx_t *c, const mi_cls_move_args_t *h, void *stream)
{
	int rc = move_check(c, h);
	if (rc)
		return rc;
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(set_device(c->device));
	rc = move_scratch(c, 0);
	if (rc)
		return rc;
	// the scratch is one move's at a time: a move on another stream follows
	// the previous one
	if (c->move_used && c->move_last != st)
		HIP_OK(hipStreamWaitEvent(st, c->move_ev, 0));
	// the table's device copy and dst_queue behind it, refreshed when the host
	// table's stamp moved
	const mi_cls_enq_tab_t *tab = h->tab;
	const uint32_t ndst = tab->ndst;
	if (!c->move_tab_src || c->move_tab_src != tab || c->move_tab_stamp != tab->stamp) {
		rc = move_idle(c);
		if (rc)
			return rc;
		memcpy(c->h_move_tab + MOVE_FIX_TAB, tab, sizeof(*tab));
		if (ndst)
			memcpy(c->h_move_tab + MOVE_FIX_DSTQ, h->dst_queue, (size_t)ndst * 8u);
		c->move_tab_src = nullptr;
		HIP_OK(hipMemcpyAsync(c->d_move_fix, c->h_move_tab, MOVE_FIX_DSTQ + (size_t)ndst * 8u,
				      hipMemcpyHostToDevice, st));
		c->move_tab_src = tab;
		c->move_tab_stamp = ((const mi_cls_enq_tab_t *)c->h_move_tab)->stamp;
	}
	MoveArgs a;
	memset(&a, 0, sizeof(a));
	a.pkts = h->pkts;
	a.pkts_bytes = h->pkts_bytes;
	a.off = h->off;
	a.len = h->len;
	a.res = h->res;
	a.dec = h->dec;
	a.idx = h->idx;
	a.pk = h->pk;
	a.tab = (const mi_cls_enq_tab_t *)(c->d_move_fix + MOVE_FIX_TAB);
	a.dstq = (const uint64_t *)(c->d_move_fix + MOVE_FIX_DSTQ);
	// the kernel reads got[0] for every record that takes none: without
	// packets, a word of the scratch that nobody uses
	a.got = h->ngot ? h->got : a.dstq;
	a.n = h->n;
	a.ngot = h->ngot;
	a.ndst = ndst;
	const uint64_t blocks = (((uint64_t)h->n + MI_CLS_MOVE_TILE - 1u) / MI_CLS_MOVE_TILE + MOVE_WAVES - 1u) /
				MOVE_WAVES;
	a.grid = (uint32_t)(blocks < MI_CLS_MOVE_GRID ? blocks : MI_CLS_MOVE_GRID);
	a.headroom = h->headroom;
	a.data_from_meta = h->data_from_meta;
	a.input = h->input;
	a.arena_lo = h->arena_lo;
	a.arena_bytes = h->arena_bytes;
	a.ctr = (unsigned long long *)(c->d_move_fix + MOVE_FIX_CTR);
	a.ent = h->ent;
	a.out = h->out;
	// this call's counters start from zero, whatever the last one left
	HIP_OK(hipMemsetAsync(a.ctr, 0, sizeof(mi_cls_move_out_t), st));
	uint32_t *last = c->last;
	last[0] = 320u + MOVE_WAVES;
	last[1] = h->n ? 2u : 1u;
	last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = a.grid;
	rc = mi_cls_launch_move(st, a, false);
	if (rc)
		return rc;
	HIP_OK(hipEventRecord(c->move_ev, st));
	c->move_used = true;
	c->move_last = st;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// The host forms' own condition: the packets are worked on in place
static int move_host_check(const mi_cls_ctx_t *c, const mi_cls_move_args_t *a)
{
	const int rc = move_check(c, a);
	if (rc)
		return rc;
	if (a->n == 0)
		return 0;
	return a->arena_bytes && mi_cls_host_mapped((const void *)(uintptr_t)a->arena_lo) &&
			       mi_cls_host_mapped((const void *)(uintptr_t)(a->arena_lo + a->arena_bytes - 1u)) ? 0 : -EINVAL;
}

// A host batch on the context's stream, nothing waited for: in place when
// every array is page-locked, else the frames, offsets and lengths through the
// staging buffers (stage_up), the records through d_out, dec, idx, got, pk and
// ent through the move's staging buffer and out through the scratch.
static int move_host_launch(mi_cls_ctx_t *c, const mi_cls_move_args_t *h)
{
	HIP_OK(set_device(c->device));
	mi_cls_move_args_t a = *h;
	const uint32_t n = h->n, ngot = h->ngot;
	if (dev_views(a.out) && (n == 0 || (dev_views(a.pkts, a.off, a.len, a.res, a.dec, a.idx, a.ent) &&
					    (!ngot || dev_views(a.got)) && (!h->pk || dev_views(a.pk))))) {
		if (n == 0)
			a.pk = nullptr;
		return mi_cls_pool_move(c, &a, c->stream);
	}
	a = *h;
	int rc = move_scratch(c, n > ngot ? (n ? n : 1u) : ngot);
	if (rc)
		return rc;
	mi_cls_move_out_t *dout = (mi_cls_move_out_t *)(c->d_move_fix + MOVE_FIX_OUT);
	if (n) {
		rc = stage_up(c, h->pkts, (size_t)h->pkts_bytes, (size_t)h->pkts_bytes, h->off, h->len, n, n);
		if (rc)
			return rc;
		HIP_OK(hipMemcpyAsync(c->d_out, h->res, n * sizeof(mi_cls_result_t), hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(move_st_dec(c), h->dec, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(move_st_idx(c), h->idx, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		if (ngot)
			HIP_OK(hipMemcpyAsync(move_st_got(c), h->got, (size_t)ngot * 8u, hipMemcpyHostToDevice, c->stream));
		if (h->pk)
			HIP_OK(hipMemcpyAsync(move_st_pk(c), h->pk, (size_t)n * 8u, hipMemcpyHostToDevice, c->stream));
		a.pkts = c->d_pk;
		a.off = c->d_off;
		a.len = c->d_len;
		a.res = c->d_out;
		a.dec = move_st_dec(c);
		a.idx = move_st_idx(c);
		a.got = ngot ? move_st_got(c) : nullptr;
		a.pk = h->pk ? move_st_pk(c) : nullptr;
		a.ent = move_st_ent(c);
	}
	a.out = dout;
	rc = mi_cls_pool_move(c, &a, c->stream);
	if (rc)
		return rc;
	if (n)
		HIP_OK(hipMemcpyAsync(h->ent, move_st_ent(c), (size_t)n * 8u, hipMemcpyDeviceToHost, c->stream));
	HIP_OK(hipMemcpyAsync(h->out, dout, sizeof(*dout), hipMemcpyDeviceToHost, c->stream));
	// the scratch is this move's until the copies have read it
	HIP_OK(hipEventRecord(c->move_ev, c->stream));
	return 0;
}

extern "C" int mi_cls_pool_move_host(mi_cls_ctx_t *c, const mi_cls_move_args_t *a)
{
	const int rc = move_host_check(c, a);
	if (rc)
		return rc;
	return host_run(c, nullptr, [&] { return move_host_launch(c, a); });
}

extern "C" int mi_cls_pool_move_host_submit(mi_cls_ctx_t *c, const mi_cls_move_args_t *a, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = move_host_check(c, a);
	if (rc)
		return rc;
	return host_run(c, ticket, [&] { return move_host_launch(c, a); });
}

extern "C" int mi_cls_pool_move_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ------------------------------------------------------------ the vector fill
// The vector fill's scratch in the context, by the pool move's policy.  Of
// fixed size: the run table's device copy, the count matrix, the counters and
// the staged form's out.  Per run: 16 B (vec_cap runs, grown by 1.5x).  The
// staged host form's arrays lie behind one another in a buffer of their own.
#define VEC_FIX_RTAB 0u
#define VEC_FIX_MAT (VEC_FIX_RTAB + ENQ_ALIGN(sizeof(mi_cls_run_tab_t)))
#define VEC_FIX_CTR (VEC_FIX_MAT + ENQ_ALIGN((size_t)(MI_CLS_RUN_VSLOTS + 1u) * MI_CLS_VEC_GRID * 4u))
#define VEC_FIX_OUT (VEC_FIX_CTR + ENQ_ALIGN(8u * 8u))
#define VEC_FIX_ROUT (VEC_FIX_OUT + ENQ_ALIGN(sizeof(mi_cls_vec_out_t)))
#define VEC_FIX_BYTES (VEC_FIX_ROUT + ENQ_ALIGN(sizeof(mi_cls_run_out_t)))
#define VEC_WAVES_PER_BLOCK (MI_CLS_VEC_TILE / 64u)

// Before the scratch is replaced, and before the table's snapshot or device
// copy is rewritten, the previous fill has ended (vec_ev).
static int vec_idle(mi_cls_ctx_t *c)
{
	if (c->vec_used)
		HIP_OK(hipEventSynchronize(c->vec_ev));
	return 0;
}

// nruns: the runs the device path keeps 16 B for; staged: bytes of the staged
// host form (0: the device path)
static int vec_scratch(mi_cls_ctx_t *c, uint32_t nruns, size_t staged)
{
	if (!c->d_vec_fix) {
		if (!c->vec_ev && hipEventCreateWithFlags(&c->vec_ev, hipEventDisableTiming) != hipSuccess)
			return -EIO;
		if ((!c->h_vec_tab &&
		     hipHostMalloc((void **)&c->h_vec_tab, sizeof(mi_cls_run_tab_t), hipHostMallocDefault) != hipSuccess) ||
		    hipMalloc((void **)&c->d_vec_fix, VEC_FIX_BYTES) != hipSuccess)
			return -ENOMEM;
	}
	if (nruns > c->vec_cap) {
		const int rc = vec_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_vec);
		c->d_vec = nullptr;
		c->vec_cap = 0;
		const size_t cap = nruns < 4096u ? 4096u : (size_t)nruns + nruns / 2;
		if (hipMalloc((void **)&c->d_vec, 16u * cap) != hipSuccess)
			return -ENOMEM;
		c->vec_cap = cap;
	}
	if (staged > c->vec_st_cap) {
		const int rc = vec_idle(c);
		if (rc)
			return rc;
		(void)hipFree(c->d_vec_st);
		c->d_vec_st = nullptr;
		c->vec_st_cap = 0;
		const size_t cap = staged < 65536u ? 65536u : staged + staged / 2;
		if (hipMalloc((void **)&c->d_vec_st, cap) != hipSuccess)
			return -ENOMEM;
		c->vec_st_cap = cap;
	}
	return 0;
}

// The table and the scalars first (host memory, no device needed), then the
// context, then the batch
static int vec_check(const mi_cls_ctx_t *c, const mi_cls_vec_args_t *a)
{
	if (!a || !a->rtab || a->n > MI_CLS_MAX_BATCH || (a->size_off & 3u) != 0 || (a->tbl_off & 7u) != 0 ||
	    (uint64_t)a->size_off + 4u > a->tbl_off || a->varena_lo + a->varena_bytes < a->varena_lo ||
	    (a->nvgot && !a->vgot))
		return -EINVAL;
	for (uint32_t s = 0; s < MI_CLS_RUN_VSLOTS; ++s)
		if ((uint64_t)a->vbase[s] + a->vhave[s] > a->nvgot)
			return -EINVAL;
	for (uint32_t i = 0; i < 256u; ++i)
		if ((a->rtab->mode[i] & MI_CLS_RUN_VEC) &&
		    (a->rtab->vmax[i] == 0 || a->rtab->vslot[i] >= MI_CLS_RUN_VSLOTS ||
		     a->rtab->vmax[i] > a->vcap[a->rtab->vslot[i]]))
			return -EINVAL;
	if (!c)
		return no_ctx();
	if (!a->out || ((uintptr_t)a->out & 7u) != 0)
		return -EINVAL;
	if (a->n == 0)
		return 0;
	if (a->run_cap && (!a->runs || !a->evr || (((uintptr_t)a->runs | (uintptr_t)a->evr) & 15u) != 0))
		return -EINVAL;
	return a->seq && a->run_out && a->ent && a->ev && a->lost &&
			       (((uintptr_t)a->ent | (uintptr_t)a->vgot | (uintptr_t)a->ev | (uintptr_t)a->lost |
				 (uintptr_t)a->run_out) & 7u) == 0 ? 0 : -EINVAL;
}

extern "C" int mi_cls_vec_fill(mi_cls_ctx_t *c, const mi_cls_vec_args_t *h, void *stream)
{
	int rc = vec_check(c, h);
	if (rc)
		return rc;
	hipStream_t st = (hipStream_t)stream;
	HIP_OK(set_device(c->device));
	// the runs the kernels can meet: the true count is on the device
	const uint32_t rb = h->run_cap < h->n ? h->run_cap : h->n;
	rc = vec_scratch(c, rb, 0);
	if (rc)
		return rc;
	// the scratch is one fill's at a time: a fill on another stream follows
	// the previous one
	if (c->vec_used && c->vec_last != st)
		HIP_OK(hipStreamWaitEvent(st, c->vec_ev, 0));
	const mi_cls_run_tab_t *rtab = h->rtab;
	if (!c->vec_tab_src || c->vec_tab_src != rtab || c->vec_tab_stamp != rtab->stamp) {
		rc = vec_idle(c);
		if (rc)
			return rc;
		memcpy(c->h_vec_tab, rtab, sizeof(*rtab));
		c->vec_tab_src = nullptr;
		HIP_OK(hipMemcpyAsync(c->d_vec_fix + VEC_FIX_RTAB, c->h_vec_tab, sizeof(*rtab), hipMemcpyHostToDevice, st));
		c->vec_tab_src = rtab;
		c->vec_tab_stamp = ((const mi_cls_run_tab_t *)c->h_vec_tab)->stamp;
	}
	VecArgs a;
	memset(&a, 0, sizeof(a));
	a.seq = h->seq;
	a.runs = h->runs;
	a.rout = h->run_out;
	a.ent = h->ent;
	a.vgot = h->vgot;
	a.rtab = (const mi_cls_run_tab_t *)(c->d_vec_fix + VEC_FIX_RTAB);
	a.n = h->n;
	a.run_cap = h->run_cap;
	a.nvgot = h->nvgot;
	a.size_off = h->size_off;
	a.tbl_off = h->tbl_off;
	{
		const uint32_t tiles = (rb + MI_CLS_VEC_TILE - 1u) / MI_CLS_VEC_TILE;
		a.grid = tiles < MI_CLS_VEC_GRID ? (tiles ? tiles : 1u) : MI_CLS_VEC_GRID;
		a.tpb = (tiles + a.grid - 1u) / a.grid;
		const uint32_t ftiles = (uint32_t)(((uint64_t)h->n + MI_CLS_VEC_TILE - 1u) / MI_CLS_VEC_TILE);
		a.fgrid = ftiles < MI_CLS_VEC_GRID ? (ftiles ? ftiles : 1u) : MI_CLS_VEC_GRID;
		a.ftpb = (ftiles + a.fgrid - 1u) / a.fgrid;
	}
	a.ent_to_handle = h->ent_to_handle;
	a.varena_lo = h->varena_lo;
	a.varena_bytes = h->varena_bytes;
	memcpy(a.vbase, h->vbase, sizeof(a.vbase));
	memcpy(a.vhave, h->vhave, sizeof(a.vhave));
	a.mat = (uint32_t *)(c->d_vec_fix + VEC_FIX_MAT);
	a.pl = (uint4 *)c->d_vec;
	a.ctr = (unsigned long long *)(c->d_vec_fix + VEC_FIX_CTR);
	a.ev = h->ev;
	a.evr = h->evr;
	a.lost = h->lost;
	a.out = h->out;
	// this call's counters start from zero, whatever the last one left
	HIP_OK(hipMemsetAsync(a.ctr, 0, 8u * 8u, st));
	uint32_t *last = c->last;
	last[0] = 384u + VEC_WAVES_PER_BLOCK;
	last[1] = h->n ? 4u : 1u;
	last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = h->n ? a.fgrid : 0u;
	rc = mi_cls_launch_vec(st, a, false);
	if (rc)
		return rc;
	HIP_OK(hipEventRecord(c->vec_ev, st));
	c->vec_used = true;
	c->vec_last = st;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// The host forms' own condition: the vectors are worked on in place
static int vec_host_check(const mi_cls_ctx_t *c, const mi_cls_vec_args_t *a)
{
	const int rc = vec_check(c, a);
	if (rc)
		return rc;
	if (a->n == 0)
		return 0;
	return a->varena_bytes && mi_cls_host_mapped((const void *)(uintptr_t)a->varena_lo) &&
			       mi_cls_host_mapped((const void *)(uintptr_t)(a->varena_lo + a->varena_bytes - 1u)) ? 0 : -EINVAL;
}

// A host batch on the context's stream, nothing waited for: in place when
// every array is page-locked, else seq, runs, the run plan's out, ent and vgot
// go up through the fill's staging buffer -- and ev, evr and lost with them, so
// that what the fill leaves alone comes back as it was -- and ev, evr, lost
// and out are copied back.
static int vec_host_launch(mi_cls_ctx_t *c, const mi_cls_vec_args_t *h)
{
	HIP_OK(set_device(c->device));
	mi_cls_vec_args_t a = *h;
	const uint32_t n = h->n, cap = h->run_cap, nv = h->nvgot;
	if (dev_views(a.out) && (n == 0 || (dev_views(a.seq, a.run_out, a.ent, a.ev, a.lost) &&
					    (!cap || dev_views(a.runs, a.evr)) && (!nv || dev_views(a.vgot)))))
		return mi_cls_vec_fill(c, &a, c->stream);
	a = *h;
	const size_t o_seq = 0, o_ent = o_seq + ENQ_ALIGN(4u * (size_t)n), o_ev = o_ent + ENQ_ALIGN(8u * (size_t)n),
		     o_lost = o_ev + ENQ_ALIGN(8u * (size_t)n), o_runs = o_lost + ENQ_ALIGN(8u * (size_t)n),
		     o_evr = o_runs + ENQ_ALIGN(16u * (size_t)cap), o_vgot = o_evr + ENQ_ALIGN(16u * (size_t)cap),
		     bytes = o_vgot + ENQ_ALIGN(8u * (size_t)nv);
	int rc = vec_scratch(c, 0, n ? bytes : 0);
	if (rc)
		return rc;
	mi_cls_vec_out_t *dout = (mi_cls_vec_out_t *)(c->d_vec_fix + VEC_FIX_OUT);
	uint8_t *d = c->d_vec_st;
	if (n) {
		// the staging buffer and the run plan's out in the scratch are the
		// previous fill's until it has ended
		if (c->vec_used && c->vec_last != c->stream)
			HIP_OK(hipStreamWaitEvent(c->stream, c->vec_ev, 0));
		HIP_OK(hipMemcpyAsync(d + o_seq, h->seq, 4u * (size_t)n, hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(d + o_ent, h->ent, 8u * (size_t)n, hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(d + o_ev, h->ev, 8u * (size_t)n, hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(d + o_lost, h->lost, 8u * (size_t)n, hipMemcpyHostToDevice, c->stream));
		if (cap) {
			HIP_OK(hipMemcpyAsync(d + o_runs, h->runs, 16u * (size_t)cap, hipMemcpyHostToDevice, c->stream));
			HIP_OK(hipMemcpyAsync(d + o_evr, h->evr, 16u * (size_t)cap, hipMemcpyHostToDevice, c->stream));
		}
		if (nv)
			HIP_OK(hipMemcpyAsync(d + o_vgot, h->vgot, 8u * (size_t)nv, hipMemcpyHostToDevice, c->stream));
		HIP_OK(hipMemcpyAsync(c->d_vec_fix + VEC_FIX_ROUT, h->run_out, sizeof(mi_cls_run_out_t),
				      hipMemcpyHostToDevice, c->stream));
		a.seq = (const uint32_t *)(d + o_seq);
		a.ent = (const uint64_t *)(d + o_ent);
		a.ev = (uint64_t *)(d + o_ev);
		a.lost = (uint64_t *)(d + o_lost);
		a.runs = cap ? (const mi_cls_run_t *)(d + o_runs) : nullptr;
		a.evr = cap ? (mi_cls_evrun_t *)(d + o_evr) : nullptr;
		a.vgot = nv ? (const uint64_t *)(d + o_vgot) : nullptr;
		a.run_out = (const mi_cls_run_out_t *)(c->d_vec_fix + VEC_FIX_ROUT);
	}
	a.out = dout;
	rc = mi_cls_vec_fill(c, &a, c->stream);
	if (rc)
		return rc;
	if (n) {
		HIP_OK(hipMemcpyAsync(h->ev, d + o_ev, 8u * (size_t)n, hipMemcpyDeviceToHost, c->stream));
		HIP_OK(hipMemcpyAsync(h->lost, d + o_lost, 8u * (size_t)n, hipMemcpyDeviceToHost, c->stream));
		if (cap)
			HIP_OK(hipMemcpyAsync(h->evr, d + o_evr, 16u * (size_t)cap, hipMemcpyDeviceToHost, c->stream));
	}
	HIP_OK(hipMemcpyAsync(h->out, dout, sizeof(*dout), hipMemcpyDeviceToHost, c->stream));
	// the scratch is this fill's until the copies have read it
	HIP_OK(hipEventRecord(c->vec_ev, c->stream));
	return 0;
}

extern "C" int mi_cls_vec_fill_host(mi_cls_ctx_t *c, const mi_cls_vec_args_t *a)
{
	const int rc = vec_host_check(c, a);
	if (rc)
		return rc;
	return host_run(c, nullptr, [&] { return vec_host_launch(c, a); });
}

extern "C" int mi_cls_vec_fill_host_submit(mi_cls_ctx_t *c, const mi_cls_vec_args_t *a, uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = vec_host_check(c, a);
	if (rc)
		return rc;
	return host_run(c, ticket, [&] { return vec_host_launch(c, a); });
}

extern "C" int mi_cls_vec_fill_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ------------------------------------------------------------------------ LSO
// _odp_lso_num_packets (odp_packet_io.c:3089-3152), its tests in its order.
extern "C" int mi_cls_lso_plan(uint32_t len, uint32_t hdr_len, uint32_t max_payload, uint32_t proto,
			       uint32_t l3, uint32_t *seg_payload, uint32_t *left_over)
{
	if (!seg_payload || !left_over)
		return -EINVAL;
	if (hdr_len > MI_CLS_LSO_MAX_PAYLOAD_OFFSET || hdr_len > len)
		return -EINVAL;
	if ((uint64_t)hdr_len + max_payload > len) {   // no segmentation needed (:3110-3116)
		*seg_payload = max_payload;
		*left_over = 0;
		return 1;
	}
	uint32_t pay = max_payload;
	if (proto == MI_CLS_LSO_PROTO_IPV4) {
		if (l3 == MI_CLS_LSO_L3_INVALID || hdr_len < l3 || hdr_len - l3 < 20u)
			return -EINVAL;
		pay &= ~7u;   // a multiple of 8 on every fragment but the last (:3133)
	}
	if (pay == 0)   // the reference divides by it (deviations)
		return -EINVAL;
	const uint32_t total = len - hdr_len;
	uint32_t num = total / pay;
	const uint32_t left = total - num * pay;
	if (left)
		++num;
	if (num > MI_CLS_LSO_MAX_SEGMENTS)
		return -EINVAL;
	*seg_payload = pay;
	*left_over = left;
	return (int)num;
}

// What odp_lso_profile_create admits (:2844-2893), of the launch's own table
static int lso_prof_check(const mi_cls_lso_profile_t *prof, uint32_t nprof)
{
	if (!prof || nprof == 0 || nprof > MI_CLS_LSO_PROFILES)
		return -EINVAL;
	for (uint32_t p = 0; p < nprof; ++p) {
		const mi_cls_lso_profile_t &q = prof[p];
		if (q.proto == 0 && q.num_custom == 0)
			continue;   // an unused slot: a descriptor naming it is refused
		if (q.proto != MI_CLS_LSO_PROTO_CUSTOM && q.proto != MI_CLS_LSO_PROTO_IPV4)
			return -EINVAL;
		if (q.num_custom > MI_CLS_LSO_MAX_CUSTOM)
			return -EINVAL;
		for (uint32_t f = 0; q.proto == MI_CLS_LSO_PROTO_CUSTOM && f < q.num_custom; ++f) {
			const mi_cls_lso_field_t &d = q.field[f];
			if (d.offset > MI_CLS_LSO_MAX_PAYLOAD_OFFSET)
				return -EINVAL;
			if (d.mod_op != MI_CLS_LSO_ADD_SEGMENT_NUM && d.mod_op != MI_CLS_LSO_WRITE_BITS)
				return -EINVAL;
			if (d.mod_op == MI_CLS_LSO_WRITE_BITS ? d.size != 1
							      : (d.size != 1 && d.size != 2 && d.size != 4 && d.size != 8))
				return -EINVAL;
		}
	}
	return 0;
}

extern "C" int mi_cls_lso_segment(mi_cls_ctx_t *c, const uint8_t *src, const uint32_t *off,
				  const uint16_t *len, const mi_cls_lso_desc_t *desc, uint32_t n,
				  uint8_t *dst, const mi_cls_lso_seg_t *seg, uint32_t nsegs,
				  const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st, void *stream)
{
	// the parameters first: a bad table is -EINVAL with or without a device
	if ((n != 0 && nsegs != 0) || prof) {
		const int rc = lso_prof_check(prof, nprof);
		if (rc)
			return rc;
	}
	if (!c)
		return no_ctx();
	if (n == 0 || nsegs == 0)
		return 0;
	if (!src || !off || !len || !desc || !dst || !seg || !st || ((uintptr_t)desc & 15u) != 0 ||
	    ((uintptr_t)seg & 7u) != 0)
		return -EINVAL;
	HIP_OK(set_device(c->device));
	LsoArgs a;
	memset(&a, 0, sizeof(a));
	a.src = src;
	a.off = off;
	a.len = len;
	a.desc = desc;
	a.dst = dst;
	a.seg = seg;
	a.st = st;
	a.n = n;
	a.nsegs = nsegs;
	a.nprof = nprof;
	memcpy(a.prof, prof, nprof * sizeof(mi_cls_lso_profile_t));
	// one wave per segment, persistent over the table: at most 8 blocks of
	// LSO_NW waves per CU (32 VGPRs: the wave slots bound it)
	const uint32_t blocks = (nsegs + LSO_NW - 1) / LSO_NW;
	const uint32_t max_grid = (uint32_t)c->num_cu * 8u;
	const uint32_t grid = blocks < max_grid ? blocks : max_grid;
	uint32_t *last = c->last;
	last[0] = 64u + LSO_NW;
	last[1] = last[2] = last[3] = last[4] = last[5] = 0;
	last[6] = grid;
	const int rc = mi_cls_launch_lso(grid, (hipStream_t)stream, a);
	if (rc)
		return rc;
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

// Segment j's length by its descriptor (valid descriptors: lso_host_check)
static uint32_t lso_seg_len(const mi_cls_lso_desc_t &d, uint32_t len, uint32_t k)
{
	return k + 1u < d.nseg ? (uint32_t)d.hdr_len + d.seg_payload
			       : len - (uint32_t)(d.nseg - 1u) * d.seg_payload;
}

// The host forms' check: the table, then every descriptor as the kernel
// expects it (mi_cls_lso_plan's result), every source inside src and every
// segment inside dst.
static int lso_host_check(const mi_cls_ctx_t *c, const uint8_t *src, size_t src_bytes, const uint32_t *off,
			  const uint16_t *len, const mi_cls_lso_desc_t *desc, uint32_t n, const uint8_t *dst,
			  size_t dst_bytes, const mi_cls_lso_seg_t *seg, uint32_t nsegs,
			  const mi_cls_lso_profile_t *prof, uint32_t nprof, const uint8_t *st)
{
	if ((n != 0 && nsegs != 0) || prof) {
		const int rc = lso_prof_check(prof, nprof);
		if (rc)
			return rc;
	}
	if (n == 0 || nsegs == 0)
		return c ? 0 : no_ctx();
	if (!src || !off || !len || !desc || !dst || !seg || !st || ((uintptr_t)desc & 15u) != 0 ||
	    ((uintptr_t)seg & 7u) != 0)
		return -EINVAL;
	if (src == dst ? src_bytes != dst_bytes
		       : (src < dst ? src + src_bytes > dst : dst + dst_bytes > src))
		return -EINVAL;
	if (!frames_inside(off, len, n, src_bytes))
		return -EINVAL;
	uint64_t owned = 0;
	for (uint32_t i = 0; i < n; ++i) {
		const mi_cls_lso_desc_t &d = desc[i];
		if (d.profile >= nprof || d.nseg < 2 ||
		    d.nseg > MI_CLS_LSO_MAX_SEGMENTS || d.hdr_len > MI_CLS_LSO_MAX_PAYLOAD_OFFSET ||
		    d.hdr_len > len[i] || d.seg_payload == 0 || (uint64_t)d.first_seg + d.nseg > nsegs)
			return -EINVAL;
		const uint32_t total = (uint32_t)len[i] - d.hdr_len, pay = d.seg_payload;
		if ((uint32_t)(d.nseg - 1u) * pay >= total || total > (uint32_t)d.nseg * pay)
			return -EINVAL;
		const uint8_t proto = prof[d.profile].proto;
		if (proto != MI_CLS_LSO_PROTO_CUSTOM &&
		    !(proto == MI_CLS_LSO_PROTO_IPV4 && (uint32_t)d.l3 + 20u <= d.hdr_len))
			return -EINVAL;
		for (uint32_t k = 0; k < d.nseg; ++k) {
			const mi_cls_lso_seg_t &s = seg[d.first_seg + k];
			if (s.src != i || (size_t)s.off + lso_seg_len(d, len[i], k) > dst_bytes)
				return -EINVAL;
		}
		owned += d.nseg;
	}
	if (owned != nsegs)
		return -EINVAL;
	if (!c)
		return no_ctx();
	return 0;
}

// A host batch on the context's stream: in place when everything is
// page-locked (nothing waited for; no 16-B rounding condition); else through
// the staging buffers -- sources, descriptors and the table up, the kernel,
// st back, and of the destination only the segments of the packets that did
// not fail (runs of adjoining segments in one copy).  The staged form has
// completed when it returns.
static int lso_host_launch(mi_cls_ctx_t *c, const uint8_t *src, size_t src_bytes, const uint32_t *off,
			   const uint16_t *len, const mi_cls_lso_desc_t *desc, uint32_t n, uint8_t *dst,
			   size_t dst_bytes, const mi_cls_lso_seg_t *seg, uint32_t nsegs,
			   const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st)
{
	HIP_OK(set_device(c->device));
	const uint8_t *zs = src;
	uint8_t *zd = dst, *zt = st;
	const uint32_t *zo = off;
	const uint16_t *zl = len;
	const mi_cls_lso_desc_t *zc = desc;
	const mi_cls_lso_seg_t *zg = seg;
	if (dev_views(zs, zd, zo, zl, zc, zg, zt))
		return mi_cls_lso_segment(c, zs, zo, zl, zc, n, zd, zg, nsegs, prof, nprof, zt, c->stream);
	const size_t dbase = stg_lso_dst(src == dst, src_bytes);
	int rc = stage_up(c, src, src_bytes, dbase + dst_bytes, off, len, n, 2u * n + nsegs);
	if (rc)
		return rc;
	hipStream_t s = c->stream;
	mi_cls_lso_desc_t *d_desc = stg_lso_desc(c);
	mi_cls_lso_seg_t *d_seg = stg_lso_seg(c, n);
	uint8_t *d_st = stg_lso_st(c, n), *d_dst = c->d_pk + dbase;
	HIP_OK(hipMemcpyAsync(d_desc, desc, n * sizeof(mi_cls_lso_desc_t), hipMemcpyHostToDevice, s));
	HIP_OK(hipMemcpyAsync(d_seg, seg, nsegs * sizeof(mi_cls_lso_seg_t), hipMemcpyHostToDevice, s));
	rc = mi_cls_lso_segment(c, c->d_pk, c->d_off, c->d_len, d_desc, n, d_dst, d_seg, nsegs, prof, nprof,
				d_st, s);
	if (rc)
		return rc;
	HIP_OK(hipMemcpyAsync(st, d_st, n, hipMemcpyDeviceToHost, s));
	HIP_OK(hipStreamSynchronize(s));
	size_t run_off = 0, run_len = 0;
	for (uint32_t i = 0; i <= n; ++i) {
		for (uint32_t k = 0; i < n && st[i] == MI_CLS_LSO_ST_OK && k < desc[i].nseg; ++k) {
			const size_t o = seg[desc[i].first_seg + k].off, l = lso_seg_len(desc[i], len[i], k);
			if (run_len && o == run_off + run_len) {
				run_len += l;
				continue;
			}
			if (run_len)
				HIP_OK(hipMemcpyAsync(dst + run_off, d_dst + run_off, run_len, hipMemcpyDeviceToHost, s));
			run_off = o;
			run_len = l;
		}
		if (i == n && run_len)
			HIP_OK(hipMemcpyAsync(dst + run_off, d_dst + run_off, run_len, hipMemcpyDeviceToHost, s));
	}
	HIP_OK(hipStreamSynchronize(s));
	return 0;
}

extern "C" int mi_cls_lso_segment_host(mi_cls_ctx_t *c, const uint8_t *src, size_t src_bytes,
				       const uint32_t *off, const uint16_t *len,
				       const mi_cls_lso_desc_t *desc, uint32_t n, uint8_t *dst, size_t dst_bytes,
				       const mi_cls_lso_seg_t *seg, uint32_t nsegs,
				       const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st)
{
	const int rc = lso_host_check(c, src, src_bytes, off, len, desc, n, dst, dst_bytes, seg, nsegs, prof, nprof, st);
	if (rc || n == 0 || nsegs == 0)
		return rc;
	return host_run(c, nullptr, [&] {
		return lso_host_launch(c, src, src_bytes, off, len, desc, n, dst, dst_bytes, seg, nsegs, prof, nprof, st);
	});
}

extern "C" int mi_cls_lso_segment_host_submit(mi_cls_ctx_t *c, const uint8_t *src, size_t src_bytes,
					      const uint32_t *off, const uint16_t *len,
					      const mi_cls_lso_desc_t *desc, uint32_t n, uint8_t *dst,
					      size_t dst_bytes, const mi_cls_lso_seg_t *seg, uint32_t nsegs,
					      const mi_cls_lso_profile_t *prof, uint32_t nprof, uint8_t *st,
					      uint64_t *ticket)
{
	if (!ticket)
		return -EINVAL;
	*ticket = 0;
	const int rc = lso_host_check(c, src, src_bytes, off, len, desc, n, dst, dst_bytes, seg, nsegs, prof, nprof, st);
	if (rc || n == 0 || nsegs == 0)
		return rc;
	return host_run(c, ticket, [&] {
		return lso_host_launch(c, src, src_bytes, off, len, desc, n, dst, dst_bytes, seg, nsegs, prof, nprof, st);
	});
}

extern "C" int mi_cls_lso_segment_host_wait(mi_cls_ctx_t *c, uint64_t ticket)
{
	return feature_host_wait(c, ticket);
}

// ---------------------------------------------------------------- multi-GPU
// the batch shards with no exchange step.  Contiguous
// slices balanced by the bytes the kernel reads per packet (min(len,128) +
// 6 B descriptor + 16 B record), one per device; concatenating the slices'
// records in device order is the single-device result, so per-queue arrival
// order is what the reference's _odp_cls_enq runs see
// (odp_classification_internal.h:208-236).
extern "C" int mi_cls_shard(const uint16_t *len, uint32_t n, uint32_t nshards, uint32_t *begin)
{
	if (!begin || nshards == 0 || (n && !len))
		return -EINVAL;
	uint64_t total = 0;
	for (uint32_t i = 0; i < n; ++i)
		total += (uint64_t)(len[i] < 128u ? len[i] : 128u) + 22u;
	begin[0] = 0;
	uint64_t cum = 0;
	uint32_t i = 0;
	for (uint32_t r = 1; r < nshards; ++r) {
		// first packet index whose running total reaches r/nshards of the
		// whole; the cut follows it
		while (i < n && (cum + (uint64_t)(len[i] < 128u ? len[i] : 128u) + 22u) * nshards <
				       total * r) {
			cum += (uint64_t)(len[i] < 128u ? len[i] : 128u) + 22u;
			++i;
		}
		begin[r] = i < n ? i + 1u : n;
		if (begin[r] < begin[r - 1])
			begin[r] = begin[r - 1];
	}
	begin[nshards] = n;
	for (uint32_t r = 1; r < nshards; ++r)
		if (begin[r] > n)
			begin[r] = n;
	return 0;
}

#define MI_GROUP_MAX 64
struct mi_cls_group {
	uint32_t n;
	mi_cls_ctx_t *ctx[MI_GROUP_MAX];
	uint32_t *begin;          // nshards + 1
	// submitted batches (mi_cls_group_classify_host_submit): one completion
	// event per context and ticket slot; busy[slot] = contexts with a slice
	hipEvent_t ev[MI_GROUP_MAX][8];
	uint64_t busy[8][MI_GROUP_MAX / 64];
	uint64_t submitted;
};

extern "C" int mi_cls_group_create(const int *devices, uint32_t n, mi_cls_group_t **out)
{
	if (!devices || !out || n == 0 || n > MI_GROUP_MAX)
		return -EINVAL;
	mi_cls_group_t *g = (mi_cls_group_t *)calloc(1, sizeof(*g));
	if (!g)
		return -ENOMEM;
	g->begin = (uint32_t *)calloc(n + 1, sizeof(uint32_t));
	if (!g->begin) {
		free(g);
		return -ENOMEM;
	}
	for (uint32_t i = 0; i < n; ++i) {
		int rc = mi_cls_ctx_create(devices[i], &g->ctx[i]);
		if (rc) {
			g->n = i;
			mi_cls_group_destroy(g);
			return rc;
		}
	}
	g->n = n;
	*out = g;
	return 0;
}

extern "C" int mi_cls_group_destroy(mi_cls_group_t *g)
{
	if (!g)
		return -EINVAL;
	for (uint32_t i = 0; i < g->n; ++i) {
		(void)hipSetDevice(g->ctx[i]->device);
		for (int t = 0; t < 8; ++t)
			if (g->ev[i][t])
				(void)hipEventDestroy(g->ev[i][t]);
		mi_cls_ctx_destroy(g->ctx[i]);
	}
	free(g->begin);
	free(g);
	return 0;
}

extern "C" uint32_t mi_cls_group_size(const mi_cls_group_t *g)
{
	return g ? g->n : 0u;
}

extern "C" mi_cls_ctx_t *mi_cls_group_ctx(mi_cls_group_t *g, uint32_t i)
{
	return g && i < g->n ? g->ctx[i] : nullptr;
}

extern "C" int mi_cls_group_rules_load(mi_cls_group_t *g, const void *tbl, size_t bytes)
{
	if (!g)
		return -EINVAL;
	for (uint32_t i = 0; i < g->n; ++i) {
		int rc = mi_cls_rules_load(g->ctx[i], tbl, bytes, nullptr);
		if (rc)
			return rc;
	}
	return 0;
}

extern "C" int mi_cls_group_pktin_opt_set(mi_cls_group_t *g, uint64_t opt)
{
	if (!g)
		return -EINVAL;
	for (uint32_t i = 0; i < g->n; ++i)
		mi_cls_pktin_opt_set(g->ctx[i], opt);
	return 0;
}

extern "C" int mi_cls_group_classify_host(mi_cls_group_t *g, const uint8_t *pkts, size_t bytes,
					  const uint32_t *off, const uint16_t *len, uint32_t n,
					  mi_cls_result_t *out)
{
	if (!g)
		return -EINVAL;
	if (n == 0)
		return 0;
	if (!pkts || !off || !len || !out)
		return -EINVAL;
	for (uint32_t k = 0; k < g->n; ++k)
		if (!g->ctx[k]->loaded)
			return -EINVAL;
	if (!frames_inside(off, len, n, bytes))
		return -EINVAL;
	int rc = mi_cls_shard(len, n, g->n, g->begin);
	if (rc)
		return rc;
	// every device's slice in flight before any wait.  Page-locked batches
	// are read in place (host_launch only enqueues work), so one thread
	// launches every slice; a pageable batch is staged by a copy the HIP
	// runtime performs synchronously, so each device gets its own host
	// thread and the slices' copies run side by side.
	int err[MI_GROUP_MAX] = { 0 };
	auto run = [&](uint32_t k, bool wait) {
		const uint32_t b = g->begin[k], e = g->begin[k + 1];
		if (b == e)
			return;
		size_t lo = off[b], hi = 0;
		for (uint32_t i = b; i < e; ++i) {
			lo = off[i] < lo ? off[i] : lo;
			hi = (size_t)off[i] + len[i] > hi ? (size_t)off[i] + len[i] : hi;
		}
		lo &= ~(size_t)15;   // keep the slice's 16-B alignment
		err[k] = host_launch(g->ctx[k], pkts, lo, hi, bytes, off + b, len + b, e - b, nullptr);
		if (err[k] || !wait)
			return;
		if (hipSetDevice(g->ctx[k]->device) != hipSuccess ||
		    hipStreamSynchronize(g->ctx[k]->stream) != hipSuccess) {
			err[k] = -EIO;
			return;
		}
		memcpy(out + b, g->ctx[k]->h_out, (size_t)(e - b) * sizeof(mi_cls_result_t));
	};
	if (dev_view(pkts) || g->n == 1) {
		for (uint32_t k = 0; k < g->n; ++k)
			run(k, false);
		for (uint32_t k = 0; k < g->n; ++k) {
			const uint32_t b = g->begin[k], e = g->begin[k + 1];
			if (b == e || err[k])
				continue;
			if (hipSetDevice(g->ctx[k]->device) != hipSuccess ||
			    hipStreamSynchronize(g->ctx[k]->stream) != hipSuccess) {
				err[k] = -EIO;
				continue;
			}
			memcpy(out + b, g->ctx[k]->h_out, (size_t)(e - b) * sizeof(mi_cls_result_t));
		}
	} else {
		std::vector<std::thread> th;
		for (uint32_t k = 1; k < g->n; ++k)
			th.emplace_back(run, k, true);
		run(0, true);
		for (auto &t : th)
			t.join();
	}
	for (uint32_t k = 0; k < g->n; ++k)
		if (err[k])
			return err[k];
	return 0;
}

// Wait for the slices of ticket slot t (those contexts' events).
static int group_wait_slot(mi_cls_group_t *g, uint64_t t)
{
	int rc = 0;
	for (uint32_t k = 0; k < g->n; ++k) {
		if (!((g->busy[t % 8][k / 64] >> (k % 64)) & 1u))
			continue;
		if (hipSetDevice(g->ctx[k]->device) != hipSuccess ||
		    hipEventSynchronize(g->ev[k][t % 8]) != hipSuccess)
			rc = -EIO;
	}
	memset(g->busy[t % 8], 0, sizeof(g->busy[t % 8]));
	return rc;
}

// Pipelined form of mi_cls_group_classify_host: every device's slice is put
// in flight and the call returns a ticket; mi_cls_group_classify_host_wait
// returns once all of the batch's records are in out_host.  Slices are read
// in place and their records written in place, so the batch, descriptors
// and records must be page-locked (mi_cls_host_alloc); otherwise the batch
// is classified synchronously here and the ticket is 0 (already done).
extern "C" int mi_cls_group_classify_host_submit(mi_cls_group_t *g, const uint8_t *pkts, size_t bytes,
						 const uint32_t *off, const uint16_t *len, uint32_t n,
						 mi_cls_result_t *out, uint64_t *ticket)
{
	if (!g || !ticket)
		return -EINVAL;
	*ticket = 0;
	if (n == 0)
		return 0;
	if (!pkts || !off || !len || !out)
		return -EINVAL;
	for (uint32_t k = 0; k < g->n; ++k)
		if (!g->ctx[k]->loaded)
			return -EINVAL;
	if (!frames_inside(off, len, n, bytes))
		return -EINVAL;
	// (otherwise host_launch would stage this batch)
	const bool inplace = dev_view(pkts) && dev_view(off) && dev_view(len) && dev_view(out) &&
			     frames_padded_inside(off, len, n, bytes);
	if (!inplace || g->n == 1)
		return g->n == 1 ? mi_cls_classify_host_submit(g->ctx[0], pkts, bytes, off, len, n, out, ticket)
				 : mi_cls_group_classify_host(g, pkts, bytes, off, len, n, out);
	int rc = mi_cls_shard(len, n, g->n, g->begin);
	if (rc)
		return rc;
	const uint64_t t = g->submitted + 1;
	rc = group_wait_slot(g, t);   // ticket t - 8: done before its slot is reused
	if (rc)
		return rc;
	for (uint32_t k = 0; k < g->n; ++k) {
		const uint32_t b = g->begin[k], e = g->begin[k + 1];
		if (b == e)
			continue;
		mi_cls_ctx_t *c = g->ctx[k];
		// descriptors keep their offsets relative to pkts (read in place)
		rc = host_launch(c, pkts, 0, bytes, bytes, off + b, len + b, e - b, out + b);
		if (!rc && !g->ev[k][t % 8] &&
		    hipEventCreateWithFlags(&g->ev[k][t % 8], hipEventDisableTiming) != hipSuccess)
			rc = -EIO;
		if (!rc && hipEventRecord(g->ev[k][t % 8], c->stream) != hipSuccess)
			rc = -EIO;
		if (rc) {
			(void)group_wait_slot(g, t);   // the slices already in flight
			return rc;
		}
		g->busy[t % 8][k / 64] |= 1ull << (k % 64);
	}
	g->submitted = t;
	*ticket = t;
	return 0;
}

extern "C" int mi_cls_group_classify_host_wait(mi_cls_group_t *g, uint64_t ticket)
{
	if (!g || ticket > g->submitted)
		return -EINVAL;
	if (g->n == 1)
		return mi_cls_classify_host_wait(g->ctx[0], ticket);
	if (ticket == 0 || ticket + 8 <= g->submitted)
		return 0;   // nothing submitted, or its slot was reused (waited for then)
	return group_wait_slot(g, ticket);
}

// pktin options for the following classify calls: odp_pktin_config_opt_t
// all_bits (checksum validation and drop-on-error bits; timestamps ignored).
extern "C" int mi_cls_batch_hint(mi_cls_ctx_t *c, uint32_t max_batch)
{
	if (!c)
		return -EINVAL;
	if (c->batch_hint == max_batch)
		return 0;
	const Shape before = pick_shape(c, c->opt);
	c->batch_hint = max_batch;
	const Shape after = pick_shape(c, c->opt);
	// the specialised kernel follows the block shape
	if (c->loaded && (before.nw != after.nw || before.lt != after.lt))
		spec_setup(c);
	return 0;
}

extern "C" int mi_cls_pktin_opt_set(mi_cls_ctx_t *c, uint64_t opt)
{
	if (!c)
		return -EINVAL;
	const bool was = c->opt != 0;
	c->opt = (uint32_t)(opt & 0x7FCull);   // bits 2..10
	// the specialised kernel follows: the option kernel's or the plain one's
	if (c->loaded && was != (c->opt != 0))
		spec_setup(c);
	return 0;
}

extern "C" void *mi_cls_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
		return nullptr;
	const void *d = dev_view_slow(p);
	if (d) {
		std::lock_guard<std::mutex> lk(g_hreg_mu);
		g_hreg[(uintptr_t)p] = HostRange{ bytes ? bytes : 1, (const uint8_t *)d - (const uint8_t *)p };
	}
	return p;
}

extern "C" void mi_cls_host_free(void *p)
{
	if (p) {
		{
			std::lock_guard<std::mutex> lk(g_hreg_mu);
			g_hreg.erase((uintptr_t)p);
		}
		(void)hipHostFree(p);
	}
}

extern "C" int mi_cls_stats_enable(mi_cls_ctx_t *c, const uint32_t mask[8])
{
	if (!c)
		return -EINVAL;
	int any = 0;
	for (int i = 0; i < 8; ++i) {
		c->stats_mask[i] = mask ? mask[i] : 0u;
		any |= c->stats_mask[i] != 0;
	}
	c->stats_on = any;
	return 0;
}

extern "C" int mi_cls_stats_read(mi_cls_ctx_t *c, uint64_t *host, uint32_t num)
{
	if (!c || !host || num > MAX_STATS_COS)
		return -EINVAL;
	HIP_OK(hipSetDevice(c->device));
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipMemcpy(host, c->d_stats, num * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return 0;
}

extern "C" int mi_cls_stats_reset(mi_cls_ctx_t *c)
{
	if (!c)
		return -EINVAL;
	HIP_OK(hipSetDevice(c->device));
	HIP_OK(hipDeviceSynchronize());
	HIP_OK(hipMemset(c->d_stats, 0, MAX_STATS_COS * sizeof(unsigned long long)));
	return 0;
}

extern "C" const char *mi_cls_strerror(int err)
{
	switch (-err) {
	case 0: return "success";
	case EINVAL: return "invalid argument or malformed rule table";
	case ENODEV: return "no such HIP device";
	case ENOMEM: return "out of device memory";
	case EIO: return "HIP runtime error";
	default: return "unknown error";
	}
}
