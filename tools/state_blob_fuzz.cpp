// state_blob_fuzz.cpp -- iqgpu_state_inspect against truncated and corrupted blobs, for a run under the host sanitizers.
// A stand-alone program: it links the HIP-free translation unit of the saved-state container and nothing else of the library, needs no
// device, and is no part of the test suite.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/state_blob_fuzz.cpp iq_tool_amd/csrc/state_blob.cpp -o state_blob_fuzz && ./state_blob_fuzz
//
// It builds a valid blob in memory (header + a body of pseudo-random bytes), then hands iqgpu_state_inspect
//   - the blob itself: accepted, with the header's figures;
//   - every truncation length from 0 to the full size less one, each from a heap block of exactly that size, so that a read past
//     the length is a read past the allocation;
//   - every single-byte corruption of the header (all 255 other values of every byte) and a flip of every byte of the body;
//   - a header whose size field says more than was handed over.
// Every one of those must be refused with IQGPU_EINVAL and a message.  Exit status 0 and no sanitizer report: passed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../iq_tool_amd/csrc/state_blob.hpp"

static char g_err[512];
int fail(int code, const char *fmt, ...)          // the library's is in abi.cpp, with the rest of the C ABI
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int g_bad = 0;
static void expect(bool ok, const char *what, size_t at)
{
    if (ok) return;
    if (g_bad++ < 20) fprintf(stderr, "FAILED: %s at %zu (last message: %s)\n", what, at, g_err);
}

// inspect on a heap copy of exactly n bytes
static int inspect_copy(const unsigned char *src, size_t n, iqgpu_state_info *info)
{
    unsigned char *p = (unsigned char *)malloc(n ? n : 1);
    if (!p) abort();
    if (n) memcpy(p, src, n);
    g_err[0] = 0;
    const int rc = iqgpu_state_inspect(n ? p : (const void *)p, n, info);
    free(p);
    return rc;
}

int main()
{
    using namespace iqgpu;
    const size_t body = 4096 + 16, total = sizeof(StateHeader) + body;
    std::vector<unsigned char> blob(total);
    uint32_t lcg = 12345u;
    for (size_t i = sizeof(StateHeader); i < total; ++i) { lcg = lcg * 1664525u + 1013904223u; blob[i] = (unsigned char)(lcg >> 24); }
    StateHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = kStateMagic; h.format_version = IQGPU_STATE_FORMAT_VERSION; h.bytes = total;
    h.fingerprint = 0x0123456789abcdefull; h.frames_in = 1000003; h.frames_out = 310078;
    memcpy(blob.data(), &h, sizeof(h));
    h.checksum = state_checksum(blob.data(), total);
    memcpy(blob.data(), &h, sizeof(h));

    iqgpu_state_info info;
    expect(inspect_copy(blob.data(), total, &info) == IQGPU_OK, "the valid blob is accepted", 0);
    expect(info.format_version == IQGPU_STATE_FORMAT_VERSION && info.bytes == total && info.fingerprint == h.fingerprint &&
           info.frames_in == h.frames_in && info.frames_out == h.frames_out && info.reserved == 0, "the header's figures", 0);
    // an unaligned blob reads the same
    {
        std::vector<unsigned char> odd(total + 1);
        memcpy(odd.data() + 1, blob.data(), total);
        expect(iqgpu_state_inspect(odd.data() + 1, total, &info) == IQGPU_OK && info.bytes == total, "an unaligned blob", 1);
    }
    expect(iqgpu_state_inspect(nullptr, total, &info) == IQGPU_EINVAL && g_err[0], "a NULL blob", 0);
    expect(iqgpu_state_inspect(blob.data(), total, nullptr) == IQGPU_EINVAL, "a NULL info", 0);

    for (size_t n = 0; n < total; ++n)
        expect(inspect_copy(blob.data(), n, &info) == IQGPU_EINVAL && g_err[0] && info.bytes == 0, "truncation is refused", n);

    std::vector<unsigned char> bad(blob);
    for (size_t i = 0; i < sizeof(StateHeader); ++i) {
        for (int v = 1; v < 256; ++v) {
            bad[i] = (unsigned char)(blob[i] ^ v);
            expect(inspect_copy(bad.data(), total, &info) == IQGPU_EINVAL && g_err[0], "a corrupted header byte is refused", i);
        }
        bad[i] = blob[i];
    }
    for (size_t i = sizeof(StateHeader); i < total; ++i) {
        bad[i] = (unsigned char)(blob[i] ^ (1u << (i % 8)));
        expect(inspect_copy(bad.data(), total, &info) == IQGPU_EINVAL && g_err[0], "a flipped body byte is refused", i);
        bad[i] = blob[i];
    }
    // a header that promises more than was handed over, with a checksum that would hold for the promised size
    {
        StateHeader g = h;
        g.bytes = total + 4096; g.checksum = 0;
        memcpy(bad.data(), &g, sizeof(g));
        expect(inspect_copy(bad.data(), total, &info) == IQGPU_EINVAL, "a size beyond the buffer is refused", total);
    }
    if (g_bad) { fprintf(stderr, "%d checks failed\n", g_bad); return 1; }
    printf("state_blob_fuzz: %zu truncations, %zu header corruptions, %zu body flips refused; ok\n", total, sizeof(StateHeader) * 255, body);
    return 0;
}
