// hip_stub_emfit.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`, `make asan-emfit`): the
// launches of kernels/emfit.hpp, beside tests/asan/hip_stub.cpp which stands in for the HIP runtime and every other kernel.
// Device memory is host memory there, so ASan checks every extent below against what emfit.cpp allocated.  The launches do
// their kernels' work in plain C++ from the rule both sides share (emfit_weight, emfit_index, emfit_axis_outside,
// emfit_axis_range: host code too): posing and rounding by the kernel's own kernels/complex_rule.hpp, then for every
// listed brick every voxel against every atom -- no tiles, no hit list, no columns, so a disagreement with the kernel's
// structure would show.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels/complex_rule.hpp"
#include "kernels/emfit.hpp"
#include "stub_access.hpp"

namespace ld {

static bool map_ok(const EmfitMap &map) {
    for (int k = 0; k < 3; k++)
        if (map.n[k] < 1 || map.n[k] > kEmfitMaxAxis || map.step[k] < kEmfitMinStep || map.step[k] > kEmfitMaxStep ||
            map.origin[k] < -kEmfitOriginBound || map.origin[k] > kEmfitOriginBound)
            return false;
    return map.voxels() <= kEmfitMaxVoxels;
}

hipError_t launch_emfit_init(ld_density_sums *rows, EmfitBox *boxes, const ld_density_sums *from, size_t n, hipStream_t) {
    if (n == 0) return hipSuccess;
    if (from) peek(from, 1);
    touch(rows, n);
    touch(boxes, n);
    for (size_t p = 0; p < n; p++) {
        rows[p] = from ? *from : ld_density_sums{0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 3; k++) boxes[p].lo[k] = INT_MAX, boxes[p].hi[k] = INT_MIN;
    }
    return hipSuccess;
}

hipError_t launch_emfit_fill(uint32_t *grid, const uint32_t *base, size_t n, size_t voxels, hipStream_t) {
    if (n == 0 || voxels == 0) return hipSuccess;
    if (base) peek(base, voxels);
    touch(grid, n * voxels);
    for (size_t p = 0; p < n; p++)
        for (size_t v = 0; v < voxels; v++) grid[p * voxels + v] = base ? base[v] : 0u;
    return hipSuccess;
}

hipError_t launch_emfit_pose(const ComplexDevice &m, const SaxsDevice &d, const EmfitMap &map, const double *poses, size_t stride, size_t n,
                             int first, int count, int4 *out, size_t out_stride, EmfitBox *boxes, ld_density_sums *rows, int *overflow,
                             hipStream_t) {
    if (n == 0 || count <= 0) return hipSuccess;
    if (n > 65535 || first < 0 || first + count > d.n_part || out_stride < (size_t)count || !map_ok(map)) return hipErrorInvalidValue;
    peek(poses, (n - 1) * stride + 7 + m.anm_rec + m.anm_lig);
    peek(d.part_atom, (size_t)d.n_part);
    peek(d.part_class, (size_t)d.n_part);
    touch(out, (n - 1) * out_stride + count);
    peek(boxes, n);   // initialised by the caller, grown
    peek(rows, n);
    peek(overflow, 1);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < count; a++) {
            if (d.part_class[first + a] >= kSaxsClasses) return hipErrorInvalidValue;
            int v[3];
            if (!posed_thousandths(m, poses + i * stride, d.part_atom[first + a], kComplexCoordBound, v)) *overflow = 1;
            bool outside = false;
            for (int k = 0; k < 3; k++) {
                if (v[k] < boxes[i].lo[k]) boxes[i].lo[k] = v[k];
                if (v[k] > boxes[i].hi[k]) boxes[i].hi[k] = v[k];
                outside = outside || emfit_axis_outside(v[k], map.origin[k], map.step[k], map.n[k]);
            }
            if (outside) rows[i].outside++;
            out[i * out_stride + a] = make_int4(v[0], v[1], v[2], (int)emfit_weight(d.part_class[first + a]));
        }
    return hipSuccess;
}

hipError_t launch_emfit_list(const EmfitMap &map, uint32_t reach, const EmfitBox *boxes, size_t n, uint2 *items, uint32_t *n_items, hipStream_t) {
    if (n == 0) return hipSuccess;
    if (!map_ok(map) || reach >= (1u << 16)) return hipErrorInvalidValue;
    peek(boxes, n);
    peek(n_items, 1);
    for (size_t p = 0; p < n; p++) {
        int lo[3], hi[3];
        bool any = true;
        for (int k = 0; k < 3 && any; k++) {
            if (boxes[p].lo[k] > boxes[p].hi[k]) any = false;
            else emfit_axis_range(boxes[p].lo[k], boxes[p].hi[k], reach, map.origin[k], map.step[k], map.n[k], &lo[k], &hi[k]);
            if (any && lo[k] > hi[k]) any = false;
        }
        if (!any) continue;
        for (int bz = lo[2] / kEmfitDepth; bz <= hi[2] / kEmfitDepth; bz++)
            for (int by = lo[1] / kEmfitBrick; by <= hi[1] / kEmfitBrick; by++)
                for (int bx = lo[0] / kEmfitBrick; bx <= hi[0] / kEmfitBrick; bx++)
                    items[(*n_items)++] = make_uint2((uint32_t)p, (uint32_t)((bz * map.bricks(1) + by) * map.bricks(0) + bx));   // ASan: within n x bricks
    }
    return hipSuccess;
}

hipError_t launch_emfit_bricks(const EmfitBricks &b, size_t groups, hipStream_t) {
    if (groups == 0) return hipSuccess;
    if (b.table.length < 1 || b.table.length > (uint32_t)kEmfitMaxTable || groups > (size_t)kEmfitMaxGroups || !map_ok(b.map)) return hipErrorInvalidValue;
    if (((unsigned long long)b.table.length << b.table.shift) != b.table.limit || (unsigned long long)b.table.reach * b.table.reach >= b.table.limit ||
        (unsigned long long)(b.table.reach + 1) * (b.table.reach + 1) < b.table.limit)
        return hipErrorInvalidValue;
    const size_t voxels = b.map.voxels(), n_bricks = b.map.n_bricks();
    peek(b.table.K, b.table.length);
    peek(b.map.E, voxels);
    peek(b.n_items, 1);
    peek(b.items, *b.n_items);
    peek(b.overflow, 1);
    if (b.base) peek(b.base, voxels);
    if (b.base_sums) peek(b.base_sums, n_bricks * 4);
    if (b.brick_sums) peek(b.brick_sums, n_bricks * 4);
    for (uint32_t item = 0; item < *b.n_items; item++) {
        const size_t pose = b.items[item].x;
        const int brick = (int)b.items[item].y;
        if ((size_t)brick >= n_bricks) return hipErrorInvalidValue;
        peek(b.atoms + pose * b.atom_stride, (size_t)b.n_atoms);
        const int i0 = brick % b.map.bricks(0) * kEmfitBrick, j0 = brick / b.map.bricks(0) % b.map.bricks(1) * kEmfitBrick,
                  k0 = brick / b.map.bricks(0) / b.map.bricks(1) * kEmfitDepth;
        unsigned long long sum[4] = {0, 0, 0, 0};
        for (int k = k0; k < k0 + kEmfitDepth && k < b.map.n[2]; k++)
            for (int j = j0; j < j0 + kEmfitBrick && j < b.map.n[1]; j++)
                for (int i = i0; i < i0 + kEmfitBrick && i < b.map.n[0]; i++) {
                    const size_t at = ((size_t)k * b.map.n[1] + j) * b.map.n[0] + i;
                    uint32_t v = b.base ? b.base[at] : 0u;
                    const int X = b.map.origin[0] + i * b.map.step[0], Y = b.map.origin[1] + j * b.map.step[1], Z = b.map.origin[2] + k * b.map.step[2];
                    for (int a = 0; a < b.n_atoms; a++) {
                        const int4 &atom = b.atoms[pose * b.atom_stride + a];
                        const int t = emfit_index(X - atom.x, Y - atom.y, Z - atom.z, b.table.shift, b.table.limit, b.table.reach);
                        if (t >= 0) v += (uint32_t)atom.w * b.table.K[t];
                    }
                    if (v >= kEmfitVoxelLimit) *b.overflow = 1;
                    sum[0] += v, sum[1] += (unsigned long long)v * v, sum[2] += (unsigned long long)v * b.map.E[at], sum[3] += b.map.E[at] ? v : 0u;
                    if (b.grid) b.grid[pose * voxels + at] = v;
                }
        ld_density_sums &row = b.rows[pose];
        uint64_t *word[4] = {&row.s, &row.ss, &row.se, &row.inside_sum};
        for (int w = 0; w < 4; w++) {
            if (b.brick_sums) b.brick_sums[(size_t)brick * 4 + w] = sum[w];
            *word[w] += sum[w] - (b.base_sums ? b.base_sums[(size_t)brick * 4 + w] : 0ull);   // modulo 2^64, as the kernel's atomics
        }
    }
    return hipSuccess;
}

}  // namespace ld
