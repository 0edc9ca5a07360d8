/*
 * pcap_unit.c -- stand-alone program over the capture file reader and dump
 * writer (odp_amd/csrc/odp_pcap.c).  Test infrastructure only: built with
 * -fsanitize=address,undefined by tests/test_pcap_cpu.py and run on its own.
 *
 *   pcap_unit MANIFEST
 * runs the manifest's lines in order:
 *   check FILE FRAMES   parse FILE's image: PCAP_OK, the frames of FRAMES
 *   load FILE FRAMES    the same through the file entry (pcap_load)
 *   code FILE N         parse FILE's image: the return code N
 *   trunc FILE          every proper prefix of FILE's image: an error code,
 *                       or a prefix of the whole file's frames
 *   exact               16384 frames of 64 B: the store's size, its last byte
 *   self                dump writer round trip, MAC filter, a missing file
 * FRAMES is a u32 count, then per frame a u32 length and the bytes (host
 * byte order).  Every image is parsed from a heap block of exactly its size,
 * so a read one byte past it is reported.  Exit status 0 and "OK" when every
 * check holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "odp_pcap.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint8_t *slurp(const char *path, size_t *size)
{
	FILE *f = fopen(path, "rb");
	long sz;

	if (!f || fseek(f, 0, SEEK_END) || (sz = ftell(f)) < 0 || fseek(f, 0, SEEK_SET)) {
		fprintf(stderr, "cannot read %s\n", path);
		exit(2);
	}
	uint8_t *b = malloc((size_t)sz);

	if ((sz && !b) || fread(b, 1, (size_t)sz, f) != (size_t)sz) {
		fprintf(stderr, "cannot read %s\n", path);
		exit(2);
	}
	fclose(f);
	*size = (size_t)sz;
	return b;
}

/* parse a copy of img[0..size) that is exactly size bytes long */
static int parse_exact(const uint8_t *img, size_t size, pcap_store_t *st, uint32_t *link)
{
	uint8_t *b = malloc(size);
	int rc;

	if (size && !b)
		exit(2);
	if (size)
		memcpy(b, img, size);
	rc = pcap_parse(b, size, st, link);
	free(b);
	return rc;
}

/* What the store promises, read byte by byte: 64 B aligned, strictly
 * increasing offsets, zeros between the frames, 64 owned zero bytes behind
 * the last one. */
static int store_ok(const pcap_store_t *st)
{
	size_t end = 0;

	if (st->n == 0) {
		CHECK(st->bytes == 0);
		return 0;
	}
	for (uint32_t i = 0; i < st->n; i++) {
		CHECK(st->off[i] % 64 == 0);
		CHECK(i == 0 ? st->off[i] == 0 : st->off[i] > st->off[i - 1]);
		CHECK(st->len[i] >= 1);
		CHECK(st->off[i] >= end);
		for (size_t k = end; k < st->off[i]; k++)
			CHECK(st->buf[k] == 0);
		end = (size_t)st->off[i] + st->len[i];
	}
	CHECK(st->bytes == ((end + 63u) & ~(size_t)63u) + 64);
	for (size_t k = end; k < st->bytes; k++)
		CHECK(st->buf[k] == 0);
	return 0;
}

/* the store's first `n` frames are those of the FRAMES image exp */
static int frames_are(const pcap_store_t *st, const uint8_t *exp, size_t exp_size, int whole)
{
	uint32_t n;
	size_t at = 4;

	CHECK(exp_size >= 4);
	memcpy(&n, exp, 4);
	if (whole)
		CHECK(st->n == n);
	CHECK(st->n <= n);
	for (uint32_t i = 0; i < st->n; i++) {
		uint32_t l;

		CHECK(at + 4 <= exp_size);
		memcpy(&l, exp + at, 4);
		at += 4;
		CHECK(at + l <= exp_size);
		if (st->len[i] != l || memcmp(st->buf + st->off[i], exp + at, l)) {
			fprintf(stderr, "frame %u differs (length %u, expected %u)\n", i, st->len[i], l);
			return 1;
		}
		at += l;
	}
	return 0;
}

static int do_check(const char *file, const char *frames, int through_file)
{
	pcap_store_t st;
	size_t size, esize;
	uint8_t *img = slurp(file, &size), *exp = slurp(frames, &esize);
	uint32_t link = 0;

	memset(&st, 0, sizeof(st));
	CHECK((through_file ? pcap_load(file, &st, &link) : parse_exact(img, size, &st, &link)) == PCAP_OK);
	CHECK(store_ok(&st) == 0);
	CHECK(frames_are(&st, exp, esize, 1) == 0);
	pcap_store_free(&st);
	CHECK(st.buf == NULL && st.n == 0 && st.bytes == 0);
	free(img);
	free(exp);
	return 0;
}

static int do_code(const char *file, int code)
{
	pcap_store_t st;
	size_t size;
	uint8_t *img = slurp(file, &size);
	uint32_t link = 0;
	int rc;

	memset(&st, 0, sizeof(st));
	rc = parse_exact(img, size, &st, &link);
	if (rc != code) {
		fprintf(stderr, "%s: code %d, expected %d\n", file, rc, code);
		return 1;
	}
	if (rc == PCAP_E_LINKTYPE)
		CHECK(link != 1);
	CHECK(store_ok(&st) == 0);
	pcap_store_free(&st);
	free(img);
	return 0;
}

static int do_trunc(const char *file)
{
	pcap_store_t full, st;
	size_t size;
	uint8_t *img = slurp(file, &size);

	memset(&full, 0, sizeof(full));
	CHECK(parse_exact(img, size, &full, NULL) == PCAP_OK);
	CHECK(full.n == 3);
	for (size_t cut = 0; cut < size; cut++) {
		memset(&st, 0, sizeof(st));
		const int rc = parse_exact(img, cut, &st, NULL);

		CHECK(rc == PCAP_OK || rc == PCAP_E_FORMAT || rc == PCAP_E_LINKTYPE || rc == PCAP_E_IO);
		CHECK(store_ok(&st) == 0);
		if (rc == PCAP_OK) {
			CHECK(st.n <= full.n);
			for (uint32_t i = 0; i < st.n; i++) {
				CHECK(st.len[i] == full.len[i] && st.off[i] == full.off[i]);
				CHECK(memcmp(st.buf + st.off[i], full.buf + full.off[i], st.len[i]) == 0);
			}
		}
		pcap_store_free(&st);
	}
	pcap_store_free(&full);
	free(img);
	return 0;
}

/* 16384 frames of 64 B fill the store's first capacity (1 MiB) exactly: the
 * zero tail is still the store's own. */
static int do_exact(void)
{
	const uint32_t n = 16384, hdr[6] = { 0xa1b2c3d4u, 0x00040002u, 0, 0, 65535, 1 };
	const size_t size = sizeof(hdr) + (size_t)n * (16 + 64);
	uint8_t *img = malloc(size), *p = img;
	pcap_store_t st;

	CHECK(img != NULL);
	memcpy(p, hdr, sizeof(hdr));
	p += sizeof(hdr);
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t rec[4] = { i, 0, 64, 64 };

		memcpy(p, rec, 16);
		memset(p + 16, (int)(1 + i % 255), 64);
		p += 16 + 64;
	}
	memset(&st, 0, sizeof(st));
	CHECK(pcap_parse(img, size, &st, NULL) == PCAP_OK);
	CHECK(st.n == n);
	CHECK(st.bytes == (1u << 20) + 64);
	CHECK(st.buf[st.bytes - 1] == 0);
	CHECK(st.off[n - 1] == (1u << 20) - 64 && st.buf[(1u << 20) - 1] == (uint8_t)(1 + (n - 1) % 255));
	CHECK(store_ok(&st) == 0);
	pcap_store_free(&st);
	free(img);
	return 0;
}

static int do_self(const char *dir)
{
	static const uint8_t mine[8] = { 0x02, 0, 0, 0, 0, 0x02, 9, 9 }, other[8] = { 0x02, 0, 0, 0, 0, 0x03, 9, 9 },
			     mcast[8] = { 0x01, 0, 0x5e, 0, 0, 1, 9, 9 };
	uint8_t a[61], b[1500];
	char path[4096 + 16];
	pcap_store_t st;
	uint32_t link = 7;
	FILE *f;

	/* the dump writer's file is one the reader takes */
	for (size_t i = 0; i < sizeof(a); i++)
		a[i] = (uint8_t)(i + 1);
	for (size_t i = 0; i < sizeof(b); i++)
		b[i] = (uint8_t)(i * 7 + 3);
	snprintf(path, sizeof(path), "%s/dump.pcap", dir);
	f = fopen(path, "wb");
	CHECK(f != NULL);
	pcap_dump_header(f);
	pcap_dump_packet(f, a, sizeof(a));
	pcap_dump_packet(f, b, sizeof(b));
	fclose(f);
	memset(&st, 0, sizeof(st));
	CHECK(pcap_load(path, &st, &link) == PCAP_OK);
	CHECK(st.n == 2 && !st.pcapng && store_ok(&st) == 0);
	CHECK(st.len[0] == sizeof(a) && memcmp(st.buf + st.off[0], a, sizeof(a)) == 0);
	CHECK(st.len[1] == sizeof(b) && memcmp(st.buf + st.off[1], b, sizeof(b)) == 0);
	pcap_store_free(&st);
	/* a file that is not there */
	snprintf(path, sizeof(path), "%s/absent.pcap", dir);
	CHECK(pcap_load(path, &st, &link) == PCAP_E_OPEN);
	CHECK(st.n == 0 && st.buf == NULL);
	/* the MAC filter (pcap.c:176-186) */
	CHECK(pcap_filter_pass(0, mine, 8) && !pcap_filter_pass(0, other, 8) && pcap_filter_pass(0, mcast, 8));
	CHECK(pcap_filter_pass(1, other, 8) && !pcap_filter_pass(0, mine, 5) && pcap_filter_pass(1, mine, 5));
	return 0;
}

int main(int argc, char **argv)
{
	char line[8192], cmd[16], x[4096], y[4096];
	FILE *m;
	int ran = 0;

	if (argc != 2 || !(m = fopen(argv[1], "r"))) {
		fprintf(stderr, "usage: pcap_unit MANIFEST\n");
		return 2;
	}
	while (fgets(line, sizeof(line), m)) {
		const int k = sscanf(line, "%15s %4095s %4095s", cmd, x, y);
		int bad;

		if (k < 1)
			continue;
		if (!strcmp(cmd, "check") && k == 3)
			bad = do_check(x, y, 0);
		else if (!strcmp(cmd, "load") && k == 3)
			bad = do_check(x, y, 1);
		else if (!strcmp(cmd, "code") && k == 3)
			bad = do_code(x, atoi(y));
		else if (!strcmp(cmd, "trunc") && k == 2)
			bad = do_trunc(x);
		else if (!strcmp(cmd, "exact") && k == 1)
			bad = do_exact();
		else if (!strcmp(cmd, "self") && k == 2)
			bad = do_self(x);
		else
			bad = 2;
		if (bad) {
			fprintf(stderr, "failed: %s", line);
			return 1;
		}
		ran++;
	}
	fclose(m);
	printf("OK %d\n", ran);
	return 0;
}
