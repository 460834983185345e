// Stand-alone harness for zmi_digest.h (the serial forms of XXH64 and SHA-256 that digest.hip's kernels and ZSTDMI_debugDigestModel
// run): built with -fsanitize=address,undefined and run by hand, not by the suite.  Every input is a heap block of exactly its
// length, so a read beyond a piece is a report.  Checks the published vectors, then prints "<kind> <length> <hex digest>" for every
// length 0 .. 300 and 65535, 65536, 65537 of the bytes x[i] = (i * 2654435761 >> 13) & 255, for comparison with hashlib / a reference.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I zstdsharp_amd/csrc tests/host/digest_harness.cpp
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "zmi_digest.h"

using namespace zmi;

static void hex(const uint8_t* d, size_t n, char* out) { for (size_t i = 0; i < n; ++i) sprintf(out + 2 * i, "%02x", d[i]); }

static int expect(unsigned kind, const char* text, const char* want)
{
    const size_t n = strlen(text);
    std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
    memcpy(in.get(), text, n);
    uint8_t d[32]; char h[65];
    if (!digest_serial(kind, in.get(), n, d)) return 1;
    if (kind == kDigestXxh64) { uint8_t be[8]; for (int i = 0; i < 8; ++i) be[i] = d[7 - i]; hex(be, 8, h); }     // (published as a number)
    else hex(d, 32, h);
    if (strcmp(h, want)) { fprintf(stderr, "kind %u \"%s\": %s, expected %s\n", kind, text, h, want); return 1; }
    return 0;
}

int main()
{
    int bad = 0;
    bad += expect(kDigestXxh64, "", "ef46db3751d8e999");
    bad += expect(kDigestXxh64, "a", "d24ec4f1a98c6e5b");
    bad += expect(kDigestXxh64, "abc", "44bc2cf5ad770999");
    bad += expect(kDigestSha256, "", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
    bad += expect(kDigestSha256, "abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
    bad += expect(kDigestSha256, "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");
    uint8_t none[32];
    if (digest_serial(0, none, 0, none) || digest_serial(3, none, 0, none) || digest_size(0) || digest_size(3) || digest_size(1) != 8 || digest_size(2) != 32) bad++;
    std::vector<size_t> lens;
    for (size_t n = 0; n <= 300; ++n) lens.push_back(n);
    lens.push_back(65535); lens.push_back(65536); lens.push_back(65537);
    for (unsigned kind = 1; kind <= 2; ++kind)
        for (size_t n : lens) {
            std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
            for (size_t i = 0; i < n; ++i) in[i] = (uint8_t)(((uint32_t)i * 2654435761u) >> 13);
            uint8_t d[32]; char h[65];
            if (!digest_serial(kind, in.get(), n, d)) { bad++; continue; }
            hex(d, digest_size(kind), h);
            printf("%u %zu %s\n", kind, n, h);
        }
    if (bad) { fprintf(stderr, "%d FAILED\n", bad); return 1; }
    fprintf(stderr, "digest harness ok\n");
    return 0;
}
