/*
 * odp_pcap.h -- capture files for the pcap pktio: the reader (classic pcap
 * and pcapng, both byte orders; it replaces libpcap, which this image does
 * not have), the dump-file writer and the driver's MAC filter.
 *
 * Plain C over memory and stdio: no ODP type, no GPU call, no environment.
 * The reader parses untrusted input; tests/rt/pcap_unit.c runs it alone under
 * the address sanitizer.
 */
#ifndef ODP_PCAP_H
#define ODP_PCAP_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define PCAP_MTU_MAX (64 * 1024)
/* behind the last frame: zero bytes the store owns (a reader of a frame's
 * header window may run that far past a short last frame) */
#define PCAP_STORE_TAIL 64u

/* The frames of a capture, packed: frame i is buf + off[i], len[i] bytes;
 * every offset is a multiple of 64, the bytes between frames are zero and
 * so are the PCAP_STORE_TAIL bytes behind the last one. */
typedef struct {
	uint8_t *buf;
	uint32_t *off;
	uint16_t *len;
	uint32_t n;           /* frames */
	size_t bytes;         /* used bytes + PCAP_STORE_TAIL, all of them in buf; 0 with no frame */
	int pcapng;           /* the file parsed last was pcapng */
	size_t cap_bytes;     /* allocated: buf, */
	uint32_t cap_n;       /* off / len */
} pcap_store_t;

enum {
	PCAP_OK = 0,
	PCAP_E_OPEN = -1,     /* the file cannot be opened (errno says why) */
	PCAP_E_IO = -2,       /* it cannot be read, or no memory */
	PCAP_E_FORMAT = -3,   /* not a pcap / pcapng file */
	PCAP_E_LINKTYPE = -4  /* a link type other than Ethernet (1) */
};

/* internal to the library that links this unit: not part of its interface */
#pragma GCC visibility push(hidden)

/* Append the frames of the capture file image buf[0..size) to *st (zeroed
 * before its first use).  A record or block that runs past the image ends
 * the read: the frames before it are kept.  Frames of length 0 or above
 * 65535 are left out.  PCAP_OK or a PCAP_E_* code; with PCAP_E_LINKTYPE
 * *link (when not NULL) is the refused link type word.  After an error the
 * store holds whatever was read before it (pcap_store_free). */
int pcap_parse(const uint8_t *buf, size_t size, pcap_store_t *st, uint32_t *link);
/* The same for a file. */
int pcap_load(const char *fname, pcap_store_t *st, uint32_t *link);
void pcap_store_free(pcap_store_t *st);

/* Dump file (classic pcap, microseconds, Ethernet): the file header; one
 * packet record, stamped with the current time.  Both flush. */
void pcap_dump_header(FILE *f);
void pcap_dump_packet(FILE *f, const uint8_t *d, uint32_t len);

#pragma GCC visibility pop

static const uint8_t pcap_mac[6] = { 0x02, 0x00, 0x00, 0x00, 0x00, 0x02 };

/* BPF "ether dst <pcap_mac> or broadcast or multicast" (pcap.c:176-186) */
static inline int pcap_filter_pass(int promisc, const uint8_t *d, uint32_t len)
{
	if (promisc)
		return 1;
	if (len < 6)
		return 0;
	return memcmp(d, pcap_mac, 6) == 0 || (d[0] & 1u);
}

#endif
