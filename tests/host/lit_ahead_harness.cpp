// Stand-alone check of zmi_lit_ahead.h: the serial literal decoders touch their Huffman stream `ahead` bytes below the position
// they decode at, and those 4 bytes must lie inside the stream whatever the position (a decoder's last steps run below the
// stream's start) and however short the stream is against the distance.  Every ptr in [-16, 1024] x every size in [16, 1024] x
// every distance the table of DESIGN 11 holds, plus the built one.  The bytes are then really read, out of an exact-size
// allocation, so that AddressSanitizer sees an offset that leaves the stream even if the range test were wrong.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "zmi_lit_ahead.h"

int main()
{
    const int aheads[] = {128, 256, 384, 512, 768, ZMI_LIT_AHEAD};
    long bad = 0, n = 0, clampedLow = 0, clampedHigh = 0, plain = 0;
    uint32_t sink = 0;
    for (int size = 16; size <= 1024; ++size) {
        uint8_t* stream = (uint8_t*)malloc((size_t)size);
        if (!stream) return 2;
        for (int i = 0; i < size; ++i) stream[i] = (uint8_t)(i * 7 + size);
        for (int ahead : aheads) {
            if (ahead % 128) { printf("distance %d is no multiple of 128\n", ahead); ++bad; }
            for (int ptr = -16; ptr <= 1024; ++ptr, ++n) {
                const int off = zmi::lit_touch_offset(ptr, size, ahead);
                if (off < 0 || off > size - 4) { if (bad++ < 10) printf("ptr %d size %d ahead %d -> %d\n", ptr, size, ahead, off); continue; }
                uint32_t v; memcpy(&v, stream + off, 4); sink ^= v;
                // inside the stream the touch is exactly `ahead` below ptr; outside it sits on the nearer end
                const int want = ptr - ahead;
                if (want >= 0 && want <= size - 4) { ++plain; if (off != want) { if (bad++ < 10) printf("ptr %d size %d ahead %d: %d, not %d\n", ptr, size, ahead, off, want); } }
                else if (want < 0) { ++clampedLow; if (off != 0) ++bad; }
                else { ++clampedHigh; if (off != size - 4) ++bad; }
            }
        }
        free(stream);
    }
    printf("lit_ahead: %ld offsets (plain %ld, low %ld, high %ld) built %d sink %08x bad=%ld\n", n, plain, clampedLow, clampedHigh, (int)ZMI_LIT_AHEAD, sink, bad);
    return bad ? 1 : 0;
}
