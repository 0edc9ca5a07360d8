/*
 * odp_pcap.c -- capture file reader and dump writer of the pcap pktio
 * (odp_pcap.h).
 *
 * Reference behaviour: platform/linux-generic/pktio/pcap.c:119-160
 * (_pcapif_init_rx: only DLT_EN10MB is accepted), :162-174 (_pcapif_init_tx),
 * :354-401 (_pcapif_dump_pkt).
 *
 * Every length read from the file is compared against what is left of the
 * image before anything is read or added with it.
 */
#include <stdlib.h>
#include <sys/time.h>

#include "odp_pcap.h"

static uint32_t rd32s(const uint8_t *p, int swap)
{
	uint32_t v;

	memcpy(&v, p, 4);
	return swap ? __builtin_bswap32(v) : v;
}

static uint16_t rd16s(const uint8_t *p, int swap)
{
	uint16_t v;

	memcpy(&v, p, 2);
	return swap ? __builtin_bswap16(v) : v;
}

/* append one frame to the packed, 64 B aligned frame store */
static int frame_add(pcap_store_t *st, const uint8_t *d, uint32_t caplen)
{
	if (caplen > 65535 || caplen == 0)
		return 0;   /* longer than the u16 descriptor: not received */
	if (st->n == st->cap_n) {
		uint32_t nn = st->cap_n ? st->cap_n * 2 : 1024;
		uint32_t *o = realloc(st->off, nn * sizeof(uint32_t));

		if (!o)
			return -1;
		st->off = o;
		uint16_t *l = realloc(st->len, nn * sizeof(uint16_t));

		if (!l)
			return -1;
		st->len = l;
		st->cap_n = nn;
	}
	const size_t used = st->n ? st->bytes - PCAP_STORE_TAIL : 0;
	const size_t need = used + ((caplen + 63u) & ~63u) + PCAP_STORE_TAIL;

	if (need > st->cap_bytes) {
		size_t nb = st->cap_bytes ? st->cap_bytes : (1u << 20);

		while (nb < need)
			nb *= 2;
		uint8_t *b = realloc(st->buf, nb);

		if (!b)
			return -1;
		memset(b + st->cap_bytes, 0, nb - st->cap_bytes);
		st->buf = b;
		st->cap_bytes = nb;
	}
	memcpy(st->buf + used, d, caplen);
	st->off[st->n] = (uint32_t)used;
	st->len[st->n] = (uint16_t)caplen;
	st->n++;
	st->bytes = need;
	return 0;
}

/* Classic pcap (0xa1b2c3d4 / 0xa1b23c4d, either byte order) and pcapng
 * (SHB / IDB / EPB / SPB / PB blocks).  Only DLT_EN10MB (1) is accepted,
 * as in _pcapif_init_rx (pcap.c:130-134). */
int pcap_parse(const uint8_t *buf, size_t sz, pcap_store_t *st, uint32_t *linkp)
{
	if (sz < 24)
		return PCAP_E_FORMAT;
	uint32_t m = rd32s(buf, 0);

	if (m == 0xa1b2c3d4u || m == 0xa1b23c4du || m == 0xd4c3b2a1u || m == 0x4d3cb2a1u) {
		int sw = (m == 0xd4c3b2a1u || m == 0x4d3cb2a1u);

		st->pcapng = 0;
		if ((rd32s(buf + 20, sw) & 0x0fffffffu) != 1u) {
			if (linkp)
				*linkp = rd32s(buf + 20, sw);
			return PCAP_E_LINKTYPE;
		}
		for (size_t p = 24; sz - p >= 16;) {
			uint32_t incl = rd32s(buf + p + 8, sw);

			if (incl > sz - p - 16)
				break;
			if (frame_add(st, buf + p + 16, incl))
				return PCAP_E_IO;
			p += 16 + (size_t)incl;
		}
		return PCAP_OK;
	}
	if (m != 0x0a0d0d0au)
		return PCAP_E_FORMAT;
	int sw = 0;
	uint32_t link[64], nif = 0, snap[64];

	st->pcapng = 1;
	for (size_t p = 0; sz - p >= 12;) {
		uint32_t type = rd32s(buf + p, sw);

		if (type == 0x0a0d0d0au) {   /* section header: byte order */
			uint32_t bom;

			memcpy(&bom, buf + p + 8, 4);
			sw = bom == 0x4d3c2b1au;
			nif = 0;
		}
		uint32_t blen = rd32s(buf + p + 4, sw);

		if (blen < 12 || blen > sz - p)
			break;
		const uint8_t *b = buf + p + 8;
		uint32_t ifc = 0, cap = 0;
		const uint8_t *d = NULL;   /* a packet block that holds its frame whole */

		if (type == 1) {                         /* interface description */
			if (blen < 20)
				break;
			if (nif < 64) {
				link[nif] = rd16s(b, sw);
				snap[nif] = rd32s(b + 4, sw);
				nif++;
			}
		} else if (type == 6 && blen >= 32) {   /* enhanced packet */
			ifc = rd32s(b, sw);
			cap = rd32s(b + 12, sw);
			if (ifc < nif && link[ifc] != 1)
				goto bad_link;
			if (cap <= blen - 32)
				d = b + 20;
		} else if (type == 3 && blen >= 16) {   /* simple packet */
			cap = rd32s(b, sw);
			if (nif && link[0] != 1)
				goto bad_link;
			if (nif && snap[0] && cap > snap[0])
				cap = snap[0];
			if (cap <= blen - 16)
				d = b + 4;
		} else if (type == 2 && blen >= 32) {   /* obsolete packet block */
			ifc = rd16s(b, sw);
			cap = rd32s(b + 12, sw);
			if (ifc < nif && link[ifc] != 1)
				goto bad_link;
			if (cap <= blen - 32)
				d = b + 20;
		}
		if (d && frame_add(st, d, cap))
			return PCAP_E_IO;
		p += blen;
		continue;
bad_link:
		if (linkp)
			*linkp = link[ifc];
		return PCAP_E_LINKTYPE;
	}
	return PCAP_OK;
}

int pcap_load(const char *fname, pcap_store_t *st, uint32_t *link)
{
	FILE *f = fopen(fname, "rb");
	uint8_t *buf = NULL;
	long sz;
	int rc = PCAP_E_IO;

	if (!f)
		return PCAP_E_OPEN;
	if (fseek(f, 0, SEEK_END) || (sz = ftell(f)) < 0 || fseek(f, 0, SEEK_SET))
		goto out;
	buf = malloc((size_t)sz + 1);
	if (!buf || fread(buf, 1, (size_t)sz, f) != (size_t)sz)
		goto out;
	rc = pcap_parse(buf, (size_t)sz, st, link);
out:
	free(buf);
	fclose(f);
	return rc;
}

void pcap_store_free(pcap_store_t *st)
{
	free(st->buf);
	free(st->off);
	free(st->len);
	memset(st, 0, sizeof(*st));
}

void pcap_dump_header(FILE *f)
{
	const uint32_t hdr[6] = { 0xa1b2c3d4u, 0x00040002u, 0, 0, PCAP_MTU_MAX, 1 };

	fwrite(hdr, sizeof(hdr), 1, f);
	fflush(f);
}

void pcap_dump_packet(FILE *f, const uint8_t *d, uint32_t len)
{
	struct timeval tv;
	uint32_t h[4];

	gettimeofday(&tv, NULL);
	h[0] = (uint32_t)tv.tv_sec;
	h[1] = (uint32_t)tv.tv_usec;
	h[2] = h[3] = len;
	fwrite(h, sizeof(h), 1, f);
	fwrite(d, 1, len, f);
	fflush(f);
}
