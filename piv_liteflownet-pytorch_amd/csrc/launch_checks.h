// Host-only argument checks and the frame-grid rule shared by the launchers of the analysis ops.  Each check returns PIVLFN_OK, or
// PIVLFN_ERR_ARG after set_error; a launcher reads `if (int rc = check_...(...)) return rc;`, in the order it wants its refusals in.
#pragma once
#include <initializer_list>
#include "common.h"

namespace pivlfn {

// a null pointer or an empty range overlaps nothing
static inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const size_t pa = reinterpret_cast<size_t>(a), pb = reinterpret_cast<size_t>(b);
    return a != nullptr && b != nullptr && na > 0 && nb > 0 && pa < pb + nb && pb < pa + na;
}

struct Span { const void *ptr; size_t bytes; const char *name; };

// "<op>: <a> overlaps <b><tail>"; tail is "" or the op's closing words, blank and bracket included
static inline int check_apart(const char *op, const Span &a, const Span &b, const char *tail = "")
{
    PIV_REQUIRE(!ranges_overlap(a.ptr, a.bytes, b.ptr, b.bytes), "%s: %s overlaps %s%s", op, a.name, b.name, tail);
    return PIVLFN_OK;
}

// Every output against every input; the first overlapping pair is refused.  Which list is walked outermost decides the message where
// two pairs overlap at once, so there are two forms and each op keeps the order it has had: input by input ...
static inline int check_alias_by_input(const char *op, std::initializer_list<Span> outs, std::initializer_list<Span> ins, const char *tail)
{
    for (const Span &in : ins)
        for (const Span &o : outs)
            if (int rc = check_apart(op, o, in, tail)) return rc;
    return PIVLFN_OK;
}

// ... or output by output
static inline int check_alias_by_output(const char *op, std::initializer_list<Span> outs, std::initializer_list<Span> ins, const char *tail)
{
    for (const Span &o : outs)
        for (const Span &in : ins)
            if (int rc = check_apart(op, o, in, tail)) return rc;
    return PIVLFN_OK;
}

// every output against every later one: "<op>: <earlier> overlaps <later>"
static inline int check_outputs_apart(const char *op, std::initializer_list<Span> outs)
{
    for (const Span *a = outs.begin(); a != outs.end(); ++a)
        for (const Span *b = a + 1; b != outs.end(); ++b)
            if (int rc = check_apart(op, *a, *b)) return rc;
    return PIVLFN_OK;
}

// the shape triple of a batch of `noun` ("pairs", "frames", "images"): all positive, a 32-bit pixel index and, where the batch is the
// grid's y dimension (batch_in_grid), at most 65535 of them
static inline int check_shape(const char *op, int B, int H, int W, const char *noun, bool batch_in_grid = true)
{
    PIV_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad shape B=%d H=%d W=%d (all must be positive)", op, B, H, W);
    PIV_REQUIRE((size_t)H * W < ((size_t)1 << 31), "%s: H*W=%zu pixels, must stay below 2^31 (32-bit pixel index)", op, (size_t)H * W);
    PIV_REQUIRE(!batch_in_grid || B <= 65535, "%s: B=%d %s, at most 65535 per call (grid y dimension)", op, B, noun);
    return PIVLFN_OK;
}

// the workspace pair: 8-byte aligned and large enough; shape_fmt and its arguments are the op's own closing words ("B=%d H=%d W=%d")
__attribute__((format(printf, 5, 6)))
static inline int check_workspace(const char *op, const void *ws, size_t ws_bytes, size_t need, const char *shape_fmt, ...)
{
    PIV_REQUIRE(((size_t)ws & 7) == 0, "%s: the workspace must be 8-byte aligned", op);
    if (ws_bytes >= need) return PIVLFN_OK;
    char shape[96];
    va_list ap;
    va_start(ap, shape_fmt);
    vsnprintf(shape, sizeof shape, shape_fmt, ap);
    va_end(ap);
    set_error("%s: workspace of %zu bytes is too small, %zu needed for %s", op, ws_bytes, need, shape);
    return PIVLFN_ERR_ARG;
}

// The frame-grid rule: blocks of FRAME_GRID_THREADS items per frame, as many as the frame has, capped at
// max(FRAME_GRID_BLOCKS / frames, FRAME_GRID_MIN_BLOCKS) -- about as many workgroups as one flat launch would have -- and a grid-stride
// loop in the kernel above the cap.  A launch that is not per frame passes frames = 1.
constexpr int FRAME_GRID_THREADS = 256, FRAME_GRID_BLOCKS = 16384, FRAME_GRID_MIN_BLOCKS = 64;
static inline unsigned frame_grid(size_t items, int frames)
{
    const size_t g = (items + FRAME_GRID_THREADS - 1) / FRAME_GRID_THREADS;
    const size_t cap = FRAME_GRID_BLOCKS / (size_t)frames > FRAME_GRID_MIN_BLOCKS ? FRAME_GRID_BLOCKS / (size_t)frames : FRAME_GRID_MIN_BLOCKS;
    return (unsigned)(g > cap ? cap : g);
}

}  // namespace pivlfn
