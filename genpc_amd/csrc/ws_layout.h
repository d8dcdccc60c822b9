// ws_layout.h -- the layout of one scratch block, written once: each piece is named at one site (pointer, element count,
// condition), the total is known before there is a block, and bind() hands the pointers out.  THE alignment rule of the
// library's scratch: a piece starts on a 256-byte boundary and takes its size rounded up to 256 bytes.
// Host code only, no HIP: a plain C++ program can include it (tests/ws_layout_check.cpp does).
#pragma once
#include <stddef.h>
#include <string.h>

namespace genpc {

class WsLayout {
public:
    static constexpr int kMaxPieces = 24;          // (the largest layout, hpr.hip's, has 17)
    static constexpr size_t up(size_t bytes) { return (bytes + 255) / 256 * 256; }
    // `count` elements of *p behind the pieces so far; p is null until bind().  A piece of 0 elements takes no room and
    // points at its successor.  False (and ok() false from then on): the layout is full, or closed by add_tail.
    template <typename T> bool add(T *&p, size_t count) { return put(&p, count * sizeof(T), true); }
    // an absent piece takes no room and its pointer stays null
    template <typename T> bool add_if(bool present, T *&p, size_t count) { p = nullptr; return present ? add(p, count) : ok_; }
    // The one exception to the rule, for the three requests that always ended unrounded and must stay the same requests (nn_forward's
    // partials, get_uvs' keys, the paint entries) -- not for new code: a LAST piece taken at its size; nothing can follow it.
    template <typename T> bool add_tail(T *&p, size_t count) { return put(&p, count * sizeof(T), false); }
    size_t bytes() const { return off_; }          // the total so far: needs no block
    bool ok() const { return ok_; }
    // base: 256-byte aligned, bytes() long.  The pieces' pointer variables must still be where add() saw them.
    void bind(void *base) const
    {
        // (a variable is a T * of some T: written as the object pointer it is)
        for (int i = 0; i < n_; i++) { char *q = (char *)base + at_[i]; memcpy(var_[i], &q, sizeof q); }
    }
private:
    bool put(void *var, size_t bytes, bool round)
    {
        memset(var, 0, sizeof(void *));
        if (n_ == kMaxPieces || closed_) return ok_ = false;
        var_[n_] = var;
        at_[n_++] = off_;
        off_ += round ? up(bytes) : bytes;
        closed_ = !round;
        return true;
    }
    void *var_[kMaxPieces];
    size_t at_[kMaxPieces], off_ = 0;
    int n_ = 0;
    bool ok_ = true, closed_ = false;
};

}  // namespace genpc
