// pieces.h -- the offset part of a staged call: a block is a row of typed pieces that the call declares in order (`auto ids = row.piece<int32_t>(n);`).  Every piece
// begins at the next multiple of Align bytes (16: the widest device load on a staged piece), `end` is one past the last piece.  A piece is an offset until its block
// is reserved -- reserving may move the block -- and then piece_at(base, p) is its typed address: nothing else computes one, so a block's host and device sides
// cannot disagree.  Plain host C++17, no HIP: tests/cpp/staging_host.cpp holds it to these rules under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

template <class T> struct Piece {
  size_t off, n;
  size_t bytes() const { return n * sizeof(T); }
  size_t end() const { return off + bytes(); }
};
template <size_t Align = 16> struct Pieces {
  static_assert(Align && !(Align & (Align - 1)), "a power of two");
  size_t end = 0;
  static size_t aligned(size_t v) { return (v + Align - 1) & ~(Align - 1); }
  template <class T> Piece<T> piece(size_t n) {
    const size_t o = aligned(end);
    end = o + n * sizeof(T);
    return Piece<T>{o, n};
  }
  size_t end_aligned() const { return aligned(end); }
};
template <class T> T *piece_at(uint8_t *base, const Piece<T> &p) { return reinterpret_cast<T *>(base + p.off); }
