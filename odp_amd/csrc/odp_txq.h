/* odp_txq.h -- the loop pktio's choice of an input queue for every packet of
 * a send call and the split of the call into runs, host side (odp_pktout.c
 * odp_pktout_send; reference pktio/loop.c:479-530 get_dest_queue and the
 * enqueue loop of loopback_send, :554-598).  Plain C without the runtime, so
 * that a stand-alone program can exercise it (tests/rt/txq_unit.c). */
#ifndef ODP_TXQ_H
#define ODP_TXQ_H

#include <stdint.h>

/* dst[i]: the loop queue of packet i.  hash != NULL: hash[i] % num_qs (the
 * GPU's flow hash, mi_cls_tx_hash_host); NULL (the pktin hash is off):
 * index % num_qs for every packet, `index` being the pktout queue of the
 * call.  num_qs in 1 .. 256. */
static inline void txq_pick(const uint32_t *hash, uint32_t n, uint32_t index, uint32_t num_qs, uint8_t *dst)
{
	const uint8_t same = (uint8_t)(index % num_qs);

	for (uint32_t i = 0; i < n; i++)
		dst[i] = hash ? (uint8_t)(hash[i] % num_qs) : same;
}

/* The end of the run of equal destinations that starts at packet i (i < n):
 * packets [i, end) go to dst[i] with one enqueue, in arrival order. */
static inline uint32_t txq_run_end(const uint8_t *dst, uint32_t n, uint32_t i)
{
	uint32_t j = i + 1;

	while (j < n && dst[j] == dst[i])
		j++;
	return j;
}

/* The whole send: enq(arg, queue, first, count) enqueues packets [first,
 * first + count) to one queue and returns how many it took (< 0: none, an
 * error).  Stops at the first run not taken whole, as the reference stops at
 * its first failed enqueue; returns the number of leading packets sent. */
typedef int (*txq_enq_fn)(void *arg, uint32_t queue, uint32_t first, uint32_t count);

static inline uint32_t txq_send_runs(const uint8_t *dst, uint32_t n, txq_enq_fn enq, void *arg)
{
	uint32_t i = 0;

	while (i < n) {
		const uint32_t end = txq_run_end(dst, n, i);
		const int r = enq(arg, dst[i], i, end - i);

		if (r > 0)
			i += (uint32_t)r;
		if (r < 0 || i < end)
			break;
	}
	return i;
}

#endif
