// state_blob.hpp -- the container of a saved chain state (iqgpu_chain_save_state, state.cpp): header, hash, validation.  Includes
// nothing of HIP and nothing of the chain: state_blob.cpp compiles alone (tools/state_blob_fuzz.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/iqgpu.h"

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));     // abi.cpp (the fuzz program: its own)

namespace iqgpu {

// [header][host words][device buffers ...], every section a multiple of 16 bytes; all integers as the host keeps them (little-endian)
constexpr uint64_t kStateMagic = 0x3154535550475149ull;          // "IQGPUST1"
struct StateHeader {
    uint64_t magic;
    uint32_t format_version, reserved;       // reserved: 0
    uint64_t bytes;                          // of the whole blob, header included
    uint64_t fingerprint;                    // state_fingerprint (state.cpp) of the chain that saved
    uint64_t frames_in, frames_out;          // iqgpu_chain_tell at the save
    uint64_t checksum;                       // state_checksum: over every other byte of the blob
    uint64_t pad;                            // 0
};
static_assert(sizeof(StateHeader) == 64 && offsetof(StateHeader, checksum) == 48, "state header layout");

// One 64-bit hash for the fingerprint and the checksum (against corruption, not against intent).  Every step is a bijection of h
// and, for a given h, one-to-one in the word: two inputs of equal length that differ in one word never collide.
struct Hash64 {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    void word(uint64_t w) { h = (h ^ w) * 0x100000001b3ull; h ^= h >> 32; }
    void f32(float v) { uint32_t b; memcpy(&b, &v, sizeof(b)); word(b); }
    void f64(double v) { uint64_t b; memcpy(&b, &v, sizeof(b)); word(b); }
    void bytes(const void *p, size_t n)      // (any alignment; a tail of fewer than 8 bytes is zero-extended, the length goes in last)
    {
        const unsigned char *s = (const unsigned char *)p;
        size_t i = 0;
        for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, s + i, 8); word(w); }
        if (i < n) { uint64_t w = 0; memcpy(&w, s + i, n - i); word(w); }
        word((uint64_t)n);
    }
};

// the checksum of a blob of `bytes` bytes (>= the header, a multiple of 8): all of it but the header's checksum word
uint64_t state_checksum(const void *blob, size_t bytes);
// magic, version, size and checksum of a blob as `who` was handed it; *h: its header.  IQGPU_EINVAL with a message that names what is wrong
int state_blob_check(const char *who, const void *blob, size_t bytes, StateHeader *h);

} // namespace iqgpu
