// zmi_digest.h — piece digests (ZSTDMI_digestPieces, ZSTDMI_contentCutsDigests; include/zstd_mi355x.h "Piece digests"):
// the two functions' serial forms, stated once.  XXH64 (seed 0: the function of zstd's frame checksum) as round / merge / finish, and
// SHA-256 (FIPS 180-4) as block, padding and finish.  digest.hip's kernels run this text with lanes around it, ZSTDMI_debugDigestModel
// and tests/host/digest_harness.cpp run it with plain loops (the harness under AddressSanitizer / UBSan).  Plain C++ without a HIP
// header.
//
// Bytes are read through a reader R: R::le64(p) / R::le32(p) read little-endian words at any alignment.  DigestBytes, the portable
// one, builds them from single bytes; a kernel passes one that uses the device's unaligned loads.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZMI_DIGEST_HD __host__ __device__
#else
#define ZMI_DIGEST_HD
#endif

namespace zmi {

constexpr unsigned kDigestXxh64 = 1, kDigestSha256 = 2;         // ZSTDMI_digest_xxh64, ZSTDMI_digest_sha256
ZMI_DIGEST_HD inline size_t digest_size(unsigned kind) { return kind == kDigestXxh64 ? 8u : kind == kDigestSha256 ? 32u : 0u; }
inline const char* digest_stage_name(unsigned kind) { return kind == kDigestXxh64 ? "digest_xxh64" : "digest_sha256"; }

struct DigestBytes {
    ZMI_DIGEST_HD static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
    ZMI_DIGEST_HD static uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
};

// ---- XXH64 ----
// A stripe is 32 bytes; accumulator j (0 .. 3) takes the stripe's word j: v = round(v, le64(stripe + 8 j)).  The whole stripes of the
// input go through the accumulators (only when there are 32 bytes or more), the other 0 .. 31 bytes through the finish.
constexpr uint64_t kXxhP1 = 0x9E3779B185EBCA87ULL, kXxhP2 = 0xC2B2AE3D27D4EB4FULL, kXxhP3 = 0x165667B19E3779F9ULL,
                   kXxhP4 = 0x85EBCA77C2B2AE63ULL, kXxhP5 = 0x27D4EB2F165667C5ULL;
ZMI_DIGEST_HD inline uint64_t xxh64_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
ZMI_DIGEST_HD inline uint64_t xxh64_round(uint64_t acc, uint64_t in) { acc += in * kXxhP2; acc = xxh64_rotl(acc, 31); return acc * kXxhP1; }
ZMI_DIGEST_HD inline uint64_t xxh64_merge(uint64_t acc, uint64_t v) { acc ^= xxh64_round(0, v); return acc * kXxhP1 + kXxhP4; }
ZMI_DIGEST_HD inline uint64_t xxh64_start(unsigned j) { return j == 0 ? kXxhP1 + kXxhP2 : j == 1 ? kXxhP2 : j == 2 ? 0 : 0 - kXxhP1; }
// v1 .. v4: the accumulators behind the whole stripes (read only when total >= 32); tail: the total & 31 bytes behind them
template <class R>
ZMI_DIGEST_HD inline uint64_t xxh64_finish(uint64_t v1, uint64_t v2, uint64_t v3, uint64_t v4, uint64_t total, const uint8_t* tail)
{
    uint64_t h;
    if (total >= 32) {
        h = xxh64_rotl(v1, 1) + xxh64_rotl(v2, 7) + xxh64_rotl(v3, 12) + xxh64_rotl(v4, 18);
        h = xxh64_merge(h, v1); h = xxh64_merge(h, v2); h = xxh64_merge(h, v3); h = xxh64_merge(h, v4);
    } else h = kXxhP5;
    h += total;
    uint32_t left = (uint32_t)(total & 31);
    while (left >= 8) { h ^= xxh64_round(0, R::le64(tail)); h = xxh64_rotl(h, 27) * kXxhP1 + kXxhP4; tail += 8; left -= 8; }
    if (left >= 4) { h ^= (uint64_t)R::le32(tail) * kXxhP1; h = xxh64_rotl(h, 23) * kXxhP2 + kXxhP3; tail += 4; left -= 4; }
    while (left) { h ^= (uint64_t)*tail * kXxhP5; h = xxh64_rotl(h, 11) * kXxhP1; tail++; left--; }
    h ^= h >> 33; h *= kXxhP2; h ^= h >> 29; h *= kXxhP3; h ^= h >> 32;
    return h;
}
// the digest's bytes: the value, little-endian (the first four are zstd's checksum field)
ZMI_DIGEST_HD inline void xxh64_store(uint64_t h, uint8_t* out) { for (int i = 0; i < 8; ++i) out[i] = (uint8_t)(h >> (8 * i)); }
inline uint64_t xxh64_serial(const uint8_t* p, uint64_t n)
{
    uint64_t v[4];
    for (unsigned j = 0; j < 4; ++j) v[j] = xxh64_start(j);
    const uint64_t stripes = n >> 5;
    for (uint64_t i = 0; i < stripes; ++i) for (unsigned j = 0; j < 4; ++j) v[j] = xxh64_round(v[j], DigestBytes::le64(p + 32 * i + 8 * j));
    return xxh64_finish<DigestBytes>(v[0], v[1], v[2], v[3], n, p + (stripes << 5));
}

// ---- SHA-256 ----
// A block is 64 bytes = sixteen big-endian words.  The message's whole blocks, then sha256_pad_blocks(n) padding blocks made of the
// n & 63 bytes left, 0x80, zeros and the length in bits as a big-endian u64: one block when n & 63 <= 55, else two.
ZMI_DIGEST_HD inline uint32_t sha256_rotr(uint32_t x, int r) { return (x >> r) | (x << (32 - r)); }
ZMI_DIGEST_HD inline void sha256_init(uint32_t h[8])
{
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}
// one block into the state.  w: the block's sixteen words, used up as the schedule's window (w[t & 15] is W[t] while round t runs).
// Every index is a constant once the loops are unrolled: in a kernel the window and the state stay in registers.
ZMI_DIGEST_HD inline void sha256_block(uint32_t h[8], uint32_t w[16])
{
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
        0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
        0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u };
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#if defined(__clang__)
#pragma unroll
#endif
    for (unsigned t = 0; t < 64; ++t) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
        const uint32_t ch = (e & f) ^ (~e & g);
        const uint32_t t1 = hh + S1 + ch + K[t] + w[t & 15];
        const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
        const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
        const uint32_t t2 = S0 + maj;
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
ZMI_DIGEST_HD inline uint32_t sha256_pad_blocks(uint64_t n) { return (n & 63) >= 56 ? 2u : 1u; }
// word t (0 .. 15) of padding block k (0 or 1) of a message of n bytes whose last n & 63 bytes are tail[0 .. n & 63)
ZMI_DIGEST_HD inline uint32_t sha256_pad_word(const uint8_t* tail, uint64_t n, uint32_t k, uint32_t t)
{
    const uint32_t rem = (uint32_t)(n & 63), last = sha256_pad_blocks(n) - 1;
    if (k == last && t == 14) return (uint32_t)(n >> 29);           // the length in bits, high word
    if (k == last && t == 15) return (uint32_t)(n << 3);
    uint32_t w = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t i = 64 * k + 4 * t + b;
        const uint32_t v = i < rem ? tail[i] : i == rem ? 0x80u : 0u;
        w = (w << 8) | v;
    }
    return w;
}
ZMI_DIGEST_HD inline void sha256_store(const uint32_t h[8], uint8_t* out)
{
    for (int i = 0; i < 8; ++i) { out[4 * i] = (uint8_t)(h[i] >> 24); out[4 * i + 1] = (uint8_t)(h[i] >> 16); out[4 * i + 2] = (uint8_t)(h[i] >> 8); out[4 * i + 3] = (uint8_t)h[i]; }
}
inline void sha256_serial(const uint8_t* p, uint64_t n, uint8_t out[32])
{
    uint32_t h[8], w[16];
    sha256_init(h);
    const uint64_t blocks = n >> 6;
    for (uint64_t i = 0; i < blocks; ++i) {
        for (unsigned t = 0; t < 16; ++t) { const uint32_t x = DigestBytes::le32(p + 64 * i + 4 * t); w[t] = __builtin_bswap32(x); }
        sha256_block(h, w);
    }
    const uint8_t* tail = p + (blocks << 6);
    for (uint32_t k = 0; k < sha256_pad_blocks(n); ++k) {
        for (unsigned t = 0; t < 16; ++t) w[t] = sha256_pad_word(tail, n, k, t);
        sha256_block(h, w);
    }
    sha256_store(h, out);
}

// one digest on the CPU -> false for a kind that is none
inline bool digest_serial(unsigned kind, const uint8_t* p, uint64_t n, uint8_t* out)
{
    if (kind == kDigestXxh64) { xxh64_store(xxh64_serial(p, n), out); return true; }
    if (kind == kDigestSha256) { sha256_serial(p, n, out); return true; }
    return false;
}

} // namespace zmi
