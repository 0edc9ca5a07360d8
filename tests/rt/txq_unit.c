/*
 * txq_unit.c -- stand-alone program over the host side of the loop pktio's
 * queue pick and run splitting (odp_amd/csrc/odp_txq.h).  Test
 * infrastructure only: built with -fsanitize=address,undefined by
 * tests/test_txq_cpu.py and run on its own.  Exit status 0 and "OK" when
 * every check holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_txq.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

/* queues that take at most room[q] more packets; what they took, in order */
struct sink {
	uint32_t room[256];
	uint32_t calls;
	uint32_t log_q[512], log_first[512], log_count[512];
	int fail_at;   /* the call that answers -1, or -1 */
};

static int sink_enq(void *arg, uint32_t queue, uint32_t first, uint32_t count)
{
	struct sink *s = arg;
	const uint32_t take = count < s->room[queue] ? count : s->room[queue];

	if ((int)s->calls == s->fail_at)
		return -1;
	s->log_q[s->calls] = queue;
	s->log_first[s->calls] = first;
	s->log_count[s->calls] = take;
	s->calls++;
	s->room[queue] -= take;
	return (int)take;
}

static struct sink *sink_new(uint32_t room)
{
	struct sink *s = calloc(1, sizeof(*s));

	for (int q = 0; s && q < 256; q++)
		s->room[q] = room;
	if (s)
		s->fail_at = -1;
	return s;
}

int main(void)
{
	/* the arrays are sized exactly, so a read or write past them is seen */
	for (uint32_t n = 1; n <= 130; n += (n < 4 || n > 126) ? 1 : 31) {
		uint32_t *hash = malloc(n * sizeof(*hash));
		uint8_t *dst = malloc(n);

		CHECK(hash && dst);
		for (uint32_t i = 0; i < n; i++)
			hash[i] = 0x9E3779B9u * (i + 1) ^ (i << 27);
		for (uint32_t nq = 1; nq <= 64; nq += nq < 5 ? 1 : 59) {
			txq_pick(hash, n, 7, nq, dst);
			for (uint32_t i = 0; i < n; i++)
				CHECK(dst[i] == hash[i] % nq);
			/* hash off: the pktout index, for every packet */
			for (uint32_t index = 0; index < 70; index += 23) {
				txq_pick(NULL, n, index, nq, dst);
				for (uint32_t i = 0; i < n; i++)
					CHECK(dst[i] == index % nq);
				CHECK(txq_run_end(dst, n, 0) == n);
			}
		}
		/* all 32 bits take part in the modulo */
		hash[0] = 0xFFFFFFFFu;
		txq_pick(hash, 1, 0, 64, dst);
		CHECK(dst[0] == 63);
		txq_pick(hash, 1, 0, 3, dst);
		CHECK(dst[0] == 0xFFFFFFFFu % 3u);
		free(hash);
		free(dst);
	}
	{
		/* runs: 0 0 1 1 1 0 2 -> [0,2) [2,5) [5,6) [6,7) */
		const uint8_t d[7] = { 0, 0, 1, 1, 1, 0, 2 };
		uint8_t *dst = malloc(7);
		struct sink *s = sink_new(100);

		CHECK(dst && s);
		memcpy(dst, d, 7);
		CHECK(txq_run_end(dst, 7, 0) == 2 && txq_run_end(dst, 7, 2) == 5 && txq_run_end(dst, 7, 5) == 6 &&
		      txq_run_end(dst, 7, 6) == 7);
		CHECK(txq_send_runs(dst, 7, sink_enq, s) == 7 && s->calls == 4);
		CHECK(s->log_q[0] == 0 && s->log_first[0] == 0 && s->log_count[0] == 2);
		CHECK(s->log_q[1] == 1 && s->log_first[1] == 2 && s->log_count[1] == 3);
		CHECK(s->log_q[2] == 0 && s->log_first[2] == 5 && s->log_count[2] == 1);
		CHECK(s->log_q[3] == 2 && s->log_first[3] == 6 && s->log_count[3] == 1);
		free(s);
		/* queue 1 takes two: the send stops inside the second run, 4 leading packets sent */
		s = sink_new(100);
		CHECK(s);
		s->room[1] = 2;
		CHECK(txq_send_runs(dst, 7, sink_enq, s) == 4 && s->calls == 2);
		free(s);
		/* a full queue at the first run: nothing sent, one call */
		s = sink_new(0);
		CHECK(s);
		CHECK(txq_send_runs(dst, 7, sink_enq, s) == 0 && s->calls == 1);
		free(s);
		/* an enqueue error ends the send with what went before */
		s = sink_new(100);
		CHECK(s);
		s->fail_at = 2;
		CHECK(txq_send_runs(dst, 7, sink_enq, s) == 5 && s->calls == 2);
		free(s);
		/* one packet; nothing */
		s = sink_new(100);
		CHECK(s);
		CHECK(txq_send_runs(dst, 1, sink_enq, s) == 1 && s->calls == 1);
		CHECK(txq_send_runs(dst, 0, sink_enq, s) == 0 && s->calls == 1);
		free(s);
		free(dst);
	}
	printf("OK\n");
	return 0;
}
