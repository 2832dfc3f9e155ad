// A device table built on first use, stated once for the PCM stages: a key, a builder, a call.
//   table_for  looks the key up in one of the context's maps; a miss runs the builder, and the record goes into the map only when whole;
//   upload     is what a builder ends with: ONE allocation of its host pieces laid back to back, filled with blocking copies -- once per
//              table and context, so the table is whole before any launch that reads it is queued -- and freed again on any failure;
//   upload_bank is the upload both mel banks share.
// Host memory that runs out is VPZ_E_NOMEM under `oom`, a HIP call that fails VPZ_E_HIP under `what`: the caller's texts.  The maps only
// grow; free_tables (vpz_context.hip) frees the allocations when the context goes.
#pragma once

#include <initializer_list>
#include <new>
#include <vector>

#include "vpz_internal.hpp"

namespace vpz {

struct HostPiece {
    const void *data;
    size_t bytes;
    void **at;  // where the piece lies on the device
};

// (an empty piece keeps a float's room, so that its pointer lies inside the allocation; nothing is copied into it)
inline int upload(Context *ctx, const char *what, DeviceTable &rec, std::initializer_list<HostPiece> pieces)
{
    size_t total = 0;
    for (const HostPiece &h : pieces) total += h.bytes ? h.bytes : sizeof(float);
    void *mem = nullptr;
    hipError_t e = hipMalloc(&mem, total);
    if (e != hipSuccess) return set_error(ctx, VPZ_E_HIP, what, e);
    char *at = static_cast<char *>(mem);
    for (const HostPiece &h : pieces) {
        if (e == hipSuccess && h.bytes) e = hipMemcpy(at, h.data, h.bytes, hipMemcpyHostToDevice);
        *h.at = at;
        at += h.bytes ? h.bytes : sizeof(float);
    }
    if (e != hipSuccess) {
        (void)hipFree(mem);
        return set_error(ctx, VPZ_E_HIP, what, e);
    }
    rec.mem = mem;
    return VPZ_OK;
}

// `build(rec)` fills a record and ends with upload(); its status, if not VPZ_OK, is the call's and nothing is kept
template <class Map, class Build>
int table_for(Context *ctx, Map &map, const typename Map::key_type &key, const char *oom, const typename Map::mapped_type **out, Build build)
{
    try {
        auto it = map.find(key);
        if (it == map.end()) {
            typename Map::mapped_type rec;
            const int rc = build(rec);
            if (rc != VPZ_OK) return rc;
            try {
                it = map.emplace(key, rec).first;
            } catch (const std::bad_alloc &) {
                (void)hipFree(rec.mem);
                throw;
            }
        }
        *out = &it->second;
        return VPZ_OK;
    } catch (const std::bad_alloc &) {
        return set_error(ctx, VPZ_E_NOMEM, oom);
    }
}

// a mel bank on the device: the bands' records [n_mels][3] -- first live bin, live bins, where the band's weights start --, the weights
// behind them.  Bank: logmel_tables.hpp's or fbank_tables.hpp's (first, count, weights)
template <class Bank>
int upload_bank(Context *ctx, const char *what, const Bank &fb, Context::LogmelBank &bk)
{
    const size_t n_mels = fb.first.size();
    std::vector<int32_t> meta(n_mels * 3);
    int32_t at = 0;
    for (size_t b = 0; b < n_mels; ++b) {
        meta[b * 3] = fb.first[b];
        meta[b * 3 + 1] = fb.count[b];
        meta[b * 3 + 2] = at;
        at += fb.count[b];
    }
    return upload(ctx, what, bk, {{meta.data(), meta.size() * sizeof(int32_t), reinterpret_cast<void **>(&bk.d_meta)},
                                  {fb.weights.data(), fb.weights.size() * sizeof(float), reinterpret_cast<void **>(&bk.d_w)}});
}

}  // namespace vpz
