// zmi_lit_ahead.h — where the serial literal decoders warm their Huffman stream ahead of the exact look-ahead loads
// (decode_lit.hip, huf_decode_stream_fs).  No HIP in here: tests/host/lit_ahead_harness.cpp sweeps it on the host.
#pragma once

// Distance, in bytes, between a lane's position in its stream and the 4 bytes it touches in every second group of 64 symbols.  A
// multiple of the 128-byte line.  A stream is read from its last byte down, about 46 bytes per 64 symbols, so 128 is two to three
// groups ahead: time enough for a miss, and what the resident streams hold warm stays a fraction of an L2 (8192 streams per XCD:
// 1 MiB of 4; DESIGN 11 has the table the value comes from).  0 = no touch.
#ifndef ZMI_LIT_AHEAD
#define ZMI_LIT_AHEAD 128
#endif
static_assert(ZMI_LIT_AHEAD >= 0 && ZMI_LIT_AHEAD % 128 == 0, "ZMI_LIT_AHEAD is a number of 128-byte lines");

namespace zmi {

// Offset, from the stream's first byte, of the 4 bytes to touch: `ahead` below ptr, and never outside the stream — the first
// block of a call starts within a few bytes of the caller's buffer and nothing below it may be read, the last one ends at it.
// ptr = offset of the 8 bytes the decoder holds (it runs a few bytes below 0 at the end of a stream); size >= 4.
// The result is in [0, size - 4] for every ptr.  (Two comparisons: one v_med3_i32.)
constexpr int lit_touch_offset(int ptr, int size, int ahead)
{
    const int t = ptr - ahead, hi = size - 4;
    return t < 0 ? 0 : t > hi ? hi : t;
}

}  // namespace zmi
