// staging.h -- the twin block of a staged call: a pinned block and its device twin of the same size, addressed by the pieces of pieces.h.  A call declares its
// pieces, reserves the block for their `end`, fills host(p), uploads the input pieces in ONE copy, hands dev(p) to its kernels and downloads the output pieces in
// ONE copy.  Grow-only; the block never synchronises except when it grows (the twins may still be read or written by what the stream holds).  When the pinned side
// is free to be written again is the user's to know: the front end's calls end synchronised, the map's asynchronous updates wait for an event (map.hip: MapUp).
#pragma once
#include "common.h"
#include "pieces.h"
#include <algorithm>

struct TwinBlock {
  PinnedBuf<uint8_t> h; DevBuf<uint8_t> d;
  // at least `bytes` in both; a block that has to grow is replaced by one of max(2 * bytes, floor)
  int reserve(svs_ctx *ctx, size_t bytes, size_t floor = 0) {
    if (h.bytes() >= bytes) return SVS_OK;
    SVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t want = std::max(bytes * 2, floor);
    SVS_HIP(ctx, h.alloc(want));
    SVS_HIP(ctx, d.alloc(want));
    return SVS_OK;
  }
  template <class T> T *host(const Piece<T> &p) const { return piece_at(h.get(), p); }
  template <class T> T *dev(const Piece<T> &p) const { return piece_at(d.get(), p); }
  // the bytes [from, to) of one side to the same place of the other, on the context's stream
  int upload(svs_ctx *ctx, size_t from, size_t to) {
    SVS_HIP(ctx, hipMemcpyAsync(d.get() + from, h.get() + from, to - from, hipMemcpyHostToDevice, ctx->stream));
    return SVS_OK;
  }
  int download(svs_ctx *ctx, size_t from, size_t to) {
    SVS_HIP(ctx, hipMemcpyAsync(h.get() + from, d.get() + from, to - from, hipMemcpyDeviceToHost, ctx->stream));
    return SVS_OK;
  }
};
