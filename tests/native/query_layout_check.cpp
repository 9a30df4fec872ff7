// query_layout_check.cpp — the ray and path queries' buffer table and staging layout
// (qt-raytracer_amd/csrc/hippt_query_layout.h) from the host (tests/test_query_layout.py).  Host-compiled:
// the product's own header, nothing else.
//
// usage: query_layout_check
//            Builds the table of every kind of query call, as the entry points of hippt_api.cpp do, and
//            lays its staging buffer out for slices of 1, 63, 64, 65 and 2^22 rays.  Prints one line
//            per (call, slice): the call's name, the slice, the total, then "slot offset bytes out" of
//            every buffer the call has.
#include <cstdio>
#include <initializer_list>

#include "hippt_query_layout.h"

namespace {
using namespace hippt::qlayout;

char caller[1];  // stands for a caller's buffer: the layout reads no pointer, it only asks whether one is there

struct Call {
    const char *name;
    std::initializer_list<Slot> slots;  // in the entry point's order
    unsigned present;                   // bit k: the call passes its k-th buffer (else null)
};

const Call kCalls[] = {
    {"closest_t", {Slot::Rays, Slot::T, Slot::Prim}, 0b011},
    {"closest_prim", {Slot::Rays, Slot::T, Slot::Prim}, 0b101},
    {"closest_both", {Slot::Rays, Slot::T, Slot::Prim}, 0b111},
    {"occlusion", {Slot::Rays, Slot::Occluded}, 0b11},
    {"hits", {Slot::Rays, Slot::Hits}, 0b11},
    {"path_segments", {Slot::Rays, Slot::Seeds, Slot::Radiance, Slot::Segments}, 0b1111},
    {"path", {Slot::Rays, Slot::Seeds, Slot::Radiance, Slot::Segments}, 0b0111},
    {"camrays_rays", {Slot::OutRays, Slot::OutSeeds}, 0b01},
    {"camrays_seeds", {Slot::OutRays, Slot::OutSeeds}, 0b10},
    {"camrays_both", {Slot::OutRays, Slot::OutSeeds}, 0b11},
};

}  // namespace

int main() {
    for (const Call &c : kCalls) {
        Table t;
        unsigned k = 0;
        for (Slot s : c.slots) t.add(s, (c.present >> k++ & 1u) ? caller : nullptr);
        if (t.n != int(c.slots.size())) return 2;
        for (size_t cap : {size_t(1), size_t(63), size_t(64), size_t(65), size_t(1) << 22}) {
            const Staging s = staging(t, cap);
            std::printf("%s %zu %zu", c.name, cap, s.total);
            for (int i = 0; i < t.n; ++i)
                if (t.b[i].ptr) std::printf(" %d %zu %zu %d", int(t.b[i].slot), s.off[i], cap * t.b[i].bytesPerRay, int(t.b[i].out));
            std::printf("\n");
        }
    }
    return 0;
}
