// TEST INFRASTRUCTURE ONLY: a stand-alone driver of hs_heightfield_probe (vehicle_host.cpp) for the sanitizer build of
// tests/test_heightfield_geometry_cpu.py.  The field's codes and row-pair table are allocated here at exactly nx * ny elements, so
// that AddressSanitizer reports any read of the contact samplers past either table.
//   argv[1]: input  -- int32 nx, ny, n_paths, n_pts; float32 x0, y0, cell, outside_z, z_scale; int16 codes [ny][nx];
//                      float32 x [n_paths][n_pts], y [n_paths][n_pts]
//   argv[2]: output -- float32 z [n], nrm [n][3], z_cached [n], nrm_cached [n][3]; uint8 inside [n]   (n = n_paths * n_pts)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/wheeledlab_amd.h"

extern "C" void hs_heightfield_probe(const WlHeightField* hf, int n_paths, int n_pts, const float* x, const float* y, float* z, float* nrm,
                                     uint8_t* inside, float* z_cached, float* nrm_cached);

static void read_all(FILE* f, void* dst, size_t bytes) {
    if (fread(dst, 1, bytes, f) != bytes) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hdr[4];
    float fp[5];
    read_all(in, hdr, sizeof hdr);
    read_all(in, fp, sizeof fp);
    const int nx = hdr[0], ny = hdr[1], n_paths = hdr[2], n_pts = hdr[3];
    const size_t cells = (size_t)nx * ny, n = (size_t)n_paths * n_pts;
    int16_t* codes = (int16_t*)malloc(cells * sizeof(int16_t));
    uint32_t* pair = (uint32_t*)malloc(cells * sizeof(uint32_t));
    read_all(in, codes, cells * sizeof(int16_t));
    std::vector<float> x(n), y(n);
    read_all(in, x.data(), n * 4);
    read_all(in, y.data(), n * 4);
    fclose(in);
    // the header's definition: pair[j][i] = code[j][i] | code[min(j + 1, ny - 1)][i] << 16
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int up = j + 1 < ny ? j + 1 : ny - 1;
            pair[(size_t)j * nx + i] = (uint32_t)(uint16_t)codes[(size_t)j * nx + i] | (uint32_t)(uint16_t)codes[(size_t)up * nx + i] << 16;
        }
    WlHeightField hf{};
    hf.height = codes;
    hf.nx = nx, hf.ny = ny;
    hf.x0 = fp[0], hf.y0 = fp[1], hf.cell = fp[2], hf.outside_z = fp[3], hf.z_scale = fp[4];
    hf.pair = pair;
    std::vector<float> z(n), nrm(3 * n), zc(n), nc(3 * n);
    std::vector<uint8_t> inside(n);
    hs_heightfield_probe(&hf, n_paths, n_pts, x.data(), y.data(), z.data(), nrm.data(), inside.data(), zc.data(), nc.data());
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(z.data(), 4, n, out);
    fwrite(nrm.data(), 4, 3 * n, out);
    fwrite(zc.data(), 4, n, out);
    fwrite(nc.data(), 4, 3 * n, out);
    fwrite(inside.data(), 1, n, out);
    fclose(out);
    free(codes);
    free(pair);
    return 0;
}
