// state_blob.cpp -- the container of a saved chain state: checksum, validation, iqgpu_state_inspect.  No HIP include, no chain: this
// translation unit compiles alone (state_blob.hpp).
#include "state_blob.hpp"

namespace iqgpu {

uint64_t state_checksum(const void *blob, size_t bytes)
{
    const unsigned char *s = (const unsigned char *)blob;
    Hash64 k;
    k.bytes(s, offsetof(StateHeader, checksum));
    const size_t rest = offsetof(StateHeader, checksum) + sizeof(uint64_t);
    k.bytes(s + rest, bytes - rest);
    return k.h;
}

int state_blob_check(const char *who, const void *blob, size_t bytes, StateHeader *h)
{
    if (!blob) return fail(IQGPU_EINVAL, "%s: NULL blob", who);
    if (bytes < sizeof(StateHeader)) return fail(IQGPU_EINVAL, "%s: %zu bytes are no saved state (the header alone is %zu)", who, bytes,
        sizeof(StateHeader));
    memcpy(h, blob, sizeof(StateHeader));                   // (the caller's buffer may have any alignment)
    if (h->magic != kStateMagic) return fail(IQGPU_EINVAL, "%s: no saved state (magic %016llx)", who, (unsigned long long)h->magic);
    if (h->format_version != IQGPU_STATE_FORMAT_VERSION) return fail(IQGPU_EINVAL, "%s: format_version %u, this library reads %d", who,
        h->format_version, IQGPU_STATE_FORMAT_VERSION);
    if (h->bytes != (uint64_t)bytes) return fail(IQGPU_EINVAL, "%s: the blob says %llu bytes, %zu were handed over (truncated?)", who,
        (unsigned long long)h->bytes, bytes);
    if (bytes % 16 != 0) return fail(IQGPU_EINVAL, "%s: a size of %zu bytes is no multiple of 16", who, bytes);
    const uint64_t sum = state_checksum(blob, bytes);
    if (h->checksum != sum) return fail(IQGPU_EINVAL, "%s: checksum %016llx, the contents give %016llx (corrupted)", who,
        (unsigned long long)h->checksum, (unsigned long long)sum);
    if (h->reserved != 0 || h->pad != 0) return fail(IQGPU_EINVAL, "%s: reserved header words are not zero", who);
    return IQGPU_OK;
}

} // namespace iqgpu

extern "C" int iqgpu_state_inspect(const void *blob, size_t bytes, iqgpu_state_info *info)
{
    if (!info) return fail(IQGPU_EINVAL, "iqgpu_state_inspect: NULL argument");
    memset(info, 0, sizeof(*info));
    iqgpu::StateHeader h;
    const int rc = iqgpu::state_blob_check("iqgpu_state_inspect", blob, bytes, &h); if (rc) return rc;
    info->format_version = h.format_version; info->bytes = h.bytes; info->fingerprint = h.fingerprint;
    info->frames_in = h.frames_in; info->frames_out = h.frames_out;
    return IQGPU_OK;
}
