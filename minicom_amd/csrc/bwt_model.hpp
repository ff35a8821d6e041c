// minicom_amd/csrc/bwt_model.hpp -- the `.bwt` member format: header, block and anchor geometry, the checks that
// need no decoding.  Plain host C++, header only, no HIP: the ONE copy that both routes use -- the host twin (host/mcom_bwt.cpp) and the
// host half of the device route (csrc/bwt.hip) -- so that the two emit the same bytes and refuse the same members.
//
//   member  = header (40 bytes) | index (index_bytes) | embedded `.rans` member (member_bytes)
//   header  = "MCBW" | version u8 = 1 | kind u8 | blk_log2 u8 | anc_log2 u8 | raw_len u64 | crc32 of the raw bytes u32 | 0 u32 |
//             index_bytes u64 | member_bytes u64
//   kind 0  plain: no index, the embedded member codes the raw bytes themselves
//   kind 1  block sorted: the embedded member codes the move-to-front ranks of the transformed blocks, raw_len of them
//   index   for block 0, 1, ..: for k = 0 .. ceil(len / 2^anc_log2) - 1: the row (u32) of the suffix that starts at text position
//           k * 2^anc_log2 of the block; entry 0 is the primary index
// Rows of a block of `len` bytes: row 0 is the empty suffix (the end of the block sorts below every byte), rows 1 .. len the suffixes in
// ascending order.  The byte of a row is the one in front of its suffix; the row of the suffix at position 0 -- the primary index -- has
// none and is left out, so the transformed block has `len` bytes: rows 0 .. len without that one.  All integers little endian.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "rans_model.hpp"

namespace mcom_bwt {

using mcom_rans::put_u32; using mcom_rans::put_u64; using mcom_rans::get_u32; using mcom_rans::get_u64;

enum { KIND_PLAIN = 0, KIND_BWT = 1 };
constexpr uint32_t BLK_LOG2 = 20, ANC_LOG2 = 12;             // what the encoders write
constexpr uint32_t BLK_LOG2_MIN = 8, BLK_LOG2_MAX = 23;      // what the decoders take (a row number and a byte share 32 bits: rows <= 2^23)
constexpr uint32_t ANC_LOG2_MIN = 4, ANC_LOG2_MAX = 23;
constexpr size_t HEADER_BYTES = 40;
constexpr uint64_t RAW_MAX = 0xFFFFFFFEull;                  // one sort record per byte, 32-bit positions and ranks
constexpr uint32_t MTF_LOG2 = 11;                            // the device's move-to-front stretch (not part of the format)

struct Header {
	uint8_t kind = KIND_PLAIN, blk_log2 = BLK_LOG2, anc_log2 = ANC_LOG2;
	uint64_t raw_len = 0, index_bytes = 0, member_bytes = 0;
	uint32_t crc = 0;
	uint64_t blk() const { return (uint64_t)1 << blk_log2; }
	uint64_t n_blocks() const { return (raw_len + blk() - 1) >> blk_log2; }
	uint64_t block_len(uint64_t b) const { const uint64_t at = b << blk_log2; return raw_len - at < blk() ? raw_len - at : blk(); }
	uint64_t anchors_of(uint64_t len) const { return (len + ((uint64_t)1 << anc_log2) - 1) >> anc_log2; }
	uint64_t anchors_full() const { return anchors_of(blk()); }              // entries of every block but the last
	uint64_t n_anchors() const { const uint64_t nb = n_blocks(); return nb ? (nb - 1) * anchors_full() + anchors_of(block_len(nb - 1)) : 0; }
};

static inline void write_header(uint8_t *p, const Header &h)
{
	memcpy(p, "MCBW", 4); p[4] = 1; p[5] = h.kind; p[6] = h.blk_log2; p[7] = h.anc_log2;
	put_u64(p + 8, h.raw_len); put_u32(p + 16, h.crc); put_u32(p + 20, 0); put_u64(p + 24, h.index_bytes); put_u64(p + 32, h.member_bytes);
}
// Everything the header says, against the member's length: true only when the member is exactly as long as it says.
static inline bool read_header(const uint8_t *p, uint64_t len, Header &h)
{
	if (len < HEADER_BYTES || memcmp(p, "MCBW", 4) || p[4] != 1) return false;
	h.kind = p[5]; h.blk_log2 = p[6]; h.anc_log2 = p[7];
	h.raw_len = get_u64(p + 8); h.crc = get_u32(p + 16); h.index_bytes = get_u64(p + 24); h.member_bytes = get_u64(p + 32);
	if (h.kind > KIND_BWT || get_u32(p + 20) != 0) return false;
	if (h.blk_log2 < BLK_LOG2_MIN || h.blk_log2 > BLK_LOG2_MAX || h.anc_log2 < ANC_LOG2_MIN || h.anc_log2 > ANC_LOG2_MAX) return false;
	if (h.raw_len > RAW_MAX) return false;
	if (h.kind == KIND_BWT && h.raw_len == 0) return false;
	const uint64_t rest = len - HEADER_BYTES;
	if (h.index_bytes != (h.kind == KIND_BWT ? 4 * h.n_anchors() : 0)) return false;
	if (h.index_bytes > rest || rest - h.index_bytes != h.member_bytes) return false;
	return h.member_bytes >= mcom_rans::HEADER_BYTES;
}
// the embedded member's own header: it must describe exactly member_bytes, raw_len symbols and, for kind 0, the same CRC
static inline bool check_embedded(const uint8_t *m, const Header &h)
{
	mcom_rans::Header rh;
	if (!mcom_rans::read_header(m, h.member_bytes, rh) || rh.raw_len != h.raw_len) return false;
	return h.kind == KIND_BWT || rh.crc == h.crc;
}
// every row of the index lies in 1 .. the length of its block
static inline bool check_index(const uint8_t *idx, const Header &h)
{
	const uint64_t nb = h.n_blocks(), af = h.anchors_full();
	for (uint64_t b = 0; b < nb; ++b) {
		const uint64_t len = h.block_len(b), na = h.anchors_of(len);
		for (uint64_t k = 0; k < na; ++k) { const uint32_t r = get_u32(idx + 4 * (b * af + k)); if (r < 1 || r > len) return false; }
	}
	return true;
}

}  // namespace mcom_bwt
