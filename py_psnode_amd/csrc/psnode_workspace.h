// A workspace is described once: each launcher that carves a caller workspace into segments has one X_layout(shape..., Arena&) that
// names them in order.  On an arena without a base the function counts (the *_workspace_bytes / *_floats / *_pack_floats query); on the
// caller's pointer it places (the launch).  Neither side adds segment sizes or offsets a pointer on its own.
#pragma once
#include <stddef.h>

namespace psnode {

struct Arena {
    float* base = nullptr;      // nullptr: count only
    size_t off = 0;             // floats handed out so far

    // floats the next take(.., align_floats) skips.  Offsets are rounded, not addresses: every caller hands in a base at least as aligned
    // as the segments it asks for (the entry points check 256 bytes)
    size_t pad(size_t align_floats) const { return (align_floats - off % align_floats) % align_floats; }
    float* take(size_t floats, size_t align_floats = 1) {
        off += pad(align_floats);
        float* p = base ? base + off : nullptr;
        off += floats;
        return p;
    }
    void slack(size_t floats) { off += floats; }      // counted, never placed: each call says what it covers
    size_t floats() const { return off; }
    size_t bytes() const { return off * sizeof(float); }
};

}  // namespace psnode
