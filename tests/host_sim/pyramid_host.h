// TEST INFRASTRUCTURE ONLY: the bound pyramid of a heightfield built on the host with the device header's own serial builders
// (wl_depth_dev.h), shared by the host builds of the depth walk (depth_host.cpp) and of the viewer (viewer_host.cpp).
#pragma once
#include <algorithm>
#include <vector>

#include "wl_depth_dev.h"

// the pyramid buffer of a field exactly as wl_heightfield_build_pyramid lays it out (header, entries, copy of the heights)
static std::vector<float> host_pyramid(const WlHeightField* hf) {
    const Pyramid py = make_pyramid(hf->nx, hf->ny);
    const int P = 1 << py.lp;
    std::vector<float> buf((size_t)pyramid_total_floats(hf->nx, hf->ny), 0.f);
    pyramid_header_serial(*hf, buf.data() + py.hdr);
    buf[0] = buf[py.hdr + kPyrMax];
    uint32_t* words = reinterpret_cast<uint32_t*>(buf.data());
    for (int L = 1; L <= py.lp; ++L)
        for (int J = 0; J < (P >> L); ++J)
            for (int I = 0; I < (P >> L); ++I)
                words[(size_t)pyramid_level_offset(py.lp, L) + (size_t)J * (P >> L) + I] = plane_cell_serial(*hf, L, I, J, buf.data() + py.hdr);
    std::copy(hf->height, hf->height + (size_t)hf->nx * hf->ny, reinterpret_cast<int16_t*>(buf.data() + py.h0));
    return buf;
}
