// emfit.cpp -- the host side of the density fit (lightdock_hip.h, "Density fit"): the quantised map, the
// kernel table made with libm, the scores, and for a complex (Complex::density_fit, Complex::simulate_density) the
// argument checks, the chunking (chunk_of), the workspace (every block laid out through device_memory.hpp's Carver) and
// the launch sequence of kernels/emfit.hpp.
#include "emfit.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "complex.hpp"

namespace ld {

uint32_t isqrt64(unsigned long long v) {
    unsigned long long r = (unsigned long long)std::sqrt((double)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return (uint32_t)r;
}

uint32_t DensityKernel::reach() const { return isqrt64((unsigned long long)limit() - 1); }

DensityKernel density_kernel(uint32_t sigma) {
    if (sigma < (uint32_t)kEmfitMinSigma || sigma > (uint32_t)kEmfitMaxSigma) throw Error(LD_ERR_INVALID, "sigma must be 300 .. 15000 thousandths");
    const unsigned long long two = 2ull * sigma * sigma;
    const unsigned long long L = (unsigned long long)std::floor((double)two * std::log(510.0)) + 1;
    DensityKernel k;
    while (((L - 1) >> k.shift) + 1 > (unsigned long long)kEmfitMaxTable) k.shift++;
    const size_t T = (size_t)(((L - 1) >> k.shift) + 1);
    if (((unsigned long long)T << k.shift) >= (1ull << 32)) throw Error(LD_ERR_INVALID, "the kernel table's limit does not fit 32 bits");  // no sigma in range
    k.table.resize(T);
    for (size_t t = 0; t < T; t++) k.table[t] = (uint32_t)std::rint(255.0 * std::exp(-(((double)t + 0.5) * (double)(1ull << k.shift)) / (double)two));
    return k;
}

Density::Density(const float *rho, const uint32_t n[3], const int32_t origin[3], const uint32_t step[3], double threshold) {
    if (!rho || !n || !origin || !step) throw Error(LD_ERR_INVALID, "null argument");
    if (!(threshold >= 0.0) || !std::isfinite(threshold)) throw Error(LD_ERR_INVALID, "threshold must be finite and >= 0");
    size_t N = 1;
    for (int k = 0; k < 3; k++) {
        if (n[k] < 1 || n[k] > (uint32_t)kEmfitMaxAxis) throw Error(LD_ERR_INVALID, "a map has 1 .. 1024 voxels an axis");
        if (step[k] < (uint32_t)kEmfitMinStep || step[k] > (uint32_t)kEmfitMaxStep) throw Error(LD_ERR_INVALID, "a voxel's step must be 200 .. 20000 thousandths");
        if (origin[k] < -kEmfitOriginBound || origin[k] > kEmfitOriginBound) throw Error(LD_ERR_INVALID, "the origin must be within +-10^9 thousandths");
        map_.n[k] = (int)n[k], map_.origin[k] = origin[k], map_.step[k] = (int)step[k];
        N *= n[k];
    }
    if (N > kEmfitMaxVoxels) throw Error(LD_ERR_INVALID, "a map has at most 2^24 voxels");
    double top = 0.0;
    for (size_t v = 0; v < N; v++) {
        if (!std::isfinite(rho[v])) throw Error(LD_ERR_INVALID, "voxel " + std::to_string(v) + " is not finite");
        const double x = (double)rho[v];
        if (x >= threshold && x > top) top = x;
    }
    if (!(top > 0.0)) throw Error(LD_ERR_INVALID, "the map holds no positive value at or above the threshold");
    scale_ = 32767.0 / top;
    E_.resize(N);
    for (size_t v = 0; v < N; v++) {
        const double x = (double)rho[v];
        const uint64_t e = x >= threshold && x > 0.0 ? (uint64_t)std::rint(x * scale_) : 0;
        E_[v] = (uint16_t)e;
        s_e_ += e;
        s_ee_ += e * e;
    }
}

int Density::min_step() const { return std::min(map_.step[0], std::min(map_.step[1], map_.step[2])); }

EmfitMap Density::device() {
    if (!map_.E) {
        reserve_exact(d_E_, E_.size() * sizeof(uint16_t));
        hip_check(hipMemcpy(d_E_.ptr, E_.data(), E_.size() * sizeof(uint16_t), hipMemcpyHostToDevice), "hipMemcpy H2D map");
        map_.E = static_cast<const uint16_t *>(d_E_.ptr);
    }
    return map_;
}

#if !defined(__HIP_DEVICE_COMPILE__)
void Density::scores(size_t n, const ld_density_sums *sums, double *cc, double *ccm, double *inside) const {
    if (n == 0) return;
    if (!sums) throw Error(LD_ERR_INVALID, "null argument");
    typedef __int128 wide;
    const wide N = (wide)E_.size(), Se = (wide)s_e_, See = (wide)s_ee_;
    const wide C = N * See - Se * Se;
    for (size_t i = 0; i < n; i++) {
        const ld_density_sums &r = sums[i];
        if (cc) cc[i] = r.ss == 0 ? 0.0 : (double)r.se / (std::sqrt((double)r.ss) * std::sqrt((double)s_ee_));
        if (ccm) {
            const wide A = N * (wide)r.se - (wide)r.s * Se, B = N * (wide)r.ss - (wide)r.s * (wide)r.s;
            ccm[i] = (B == 0 || C == 0) ? 0.0 : (double)A / (std::sqrt((double)B) * std::sqrt((double)C));
        }
        if (inside) inside[i] = r.s == 0 ? 0.0 : (double)r.inside_sum / (double)r.s;
    }
}
#endif

// --- a complex ---------------------------------------------------------------------------------------------------------

void Complex::density_fit(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, ld_density_sums *out) {
    if (n && !out) throw Error(LD_ERR_INVALID, "null argument");
    density_run(map, n, poses, stride, sigma, out, nullptr);
}

void Complex::simulate_density(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, uint32_t *grid) {
    if (n && !grid) throw Error(LD_ERR_INVALID, "null argument");
    if (n && n > kClusterWorkspaceBytes / sizeof(uint32_t) / map.voxels()) throw Error(LD_ERR_INVALID, "more than 256 MiB of simulated voxels: ask for fewer poses a call");
    density_run(map, n, poses, stride, sigma, nullptr, grid);
}

// The sums of n poses in chunks and, with grid, their voxels.  Nothing reaches the caller before the overflow word and
// every s are known.
void Complex::density_run(Density &map, size_t n, const double *poses, size_t stride, uint32_t sigma, ld_density_sums *out, uint32_t *grid) {
    const DensityKernel kernel = density_kernel(sigma);
    if (isqrt64(kernel.limit()) > (unsigned long long)kEmfitReachVoxels * (unsigned long long)map.min_step())
        throw Error(LD_ERR_INVALID, "the kernel's support is wider than 16 voxels: the map is far finer than this resolution needs, bin it");
    const SaxsDevice &d = saxs_;
    if (d.n_part == 0) throw Error(LD_ERR_INVALID, "no atom of the complex takes part in the density (none of H, C, N, O, P, S outside MMB residues)");
    if (d.n_part > kEmfitMaxAtoms) throw Error(LD_ERR_INVALID, "more than 65536 atoms take part: a voxel would not fit 32 bits");
    if (n == 0) return;
    check_poses(n, poses, stride);
    // without receptor modes the receptor's density is the same for every pose: one base grid a call
    const bool rigid = dev_.anm_rec == 0 && d.n_part_rec >= 1;
    const int first = rigid ? d.n_part_rec : 0, count = d.n_part - first;
    const size_t N = map.voxels(), atom_bytes = (size_t)std::max(count, 1) * sizeof(int4);
    EmfitBricks b;
    b.map = map.device();
    const size_t n_bricks = b.map.n_bricks();
    const size_t per_pose = atom_bytes + n_bricks * sizeof(uint2) + sizeof(ld_density_sums) + sizeof(EmfitBox) + (grid ? N * sizeof(uint32_t) : 0);
    const size_t chunk = density_chunk_ ? std::min(density_chunk_, std::min<size_t>(n, 65535)) : chunk_of(per_pose, n, 65535);
    std::vector<ld_density_sums> h_rows(n);
    std::vector<uint32_t> h_grid(grid ? n * N : 0);
    std::vector<uint8_t> table(kernel.table.begin(), kernel.table.end());

    upload_poses(n, poses, stride);
    int4 *d_atoms, *d_rec_atoms;
    ld_density_sums *d_rows;
    EmfitBox *d_boxes;
    uint2 *d_items;
    int *d_overflow;
    uint32_t *d_n_items, *d_base, *d_grid;
    uint8_t *d_table;
    unsigned long long *d_base_sums;
    // what only a rigid receptor or only `grid` needs has no elements, and so is null, without it
    carve_into(d_ws_, [&](Carver &c) { d_atoms = c.take<int4>(chunk * (size_t)std::max(count, 1)), d_rec_atoms = c.take<int4>(rigid ? (size_t)d.n_part_rec : 0); });
    carve_into(d_out_, [&](Carver &c) {
        d_rows = c.take<ld_density_sums>(chunk + 1), d_boxes = c.take<EmfitBox>(chunk + 1);  // row and box `chunk` are the base's
        d_items = c.take<uint2>((chunk + 1) * n_bricks), d_overflow = c.take<int>(1), d_n_items = c.take<uint32_t>(1);
        d_table = c.take<uint8_t>(table.size()), d_base_sums = c.take<unsigned long long>(rigid ? n_bricks * 4 : 0);
    });
    carve_into(d_density_, [&](Carver &c) { d_base = c.take<uint32_t>(rigid ? N : 0), d_grid = c.take<uint32_t>(grid ? chunk * N : 0); });
    ld_density_sums *d_base_row = d_rows + chunk;
    EmfitBox *d_base_box = d_boxes + chunk;
    hip_check(hipMemcpyAsync(d_table, table.data(), table.size(), hipMemcpyHostToDevice, stream_), "hipMemcpy H2D table");
    const double *d_poses = static_cast<const double *>(d_poses_.ptr);
    b.table.shift = kernel.shift;
    b.table.length = (uint32_t)kernel.table.size();
    b.table.limit = kernel.limit();
    b.table.reach = kernel.reach();
    b.table.K = d_table;
    b.items = d_items;
    b.n_items = d_n_items;
    b.overflow = d_overflow;
    auto groups = [&](size_t m) { return std::min<size_t>(m * n_bricks, (size_t)kEmfitMaxGroups); };
    begin_timed(d_overflow);
    if (rigid) {
        // the receptor once: its voxels into the base grid, its sums brick by brick into the table, their totals into the base row
        hip_check(hipMemsetAsync(d_base, 0, N * sizeof(uint32_t), stream_), "hipMemset");
        hip_check(hipMemsetAsync(d_base_sums, 0, n_bricks * 4 * sizeof(unsigned long long), stream_), "hipMemset");
        hip_check(hipMemsetAsync(d_n_items, 0, sizeof(uint32_t), stream_), "hipMemset");
        hip_check(launch_emfit_init(d_base_row, d_base_box, nullptr, 1, stream_), "emfit_init launch");
        hip_check(launch_emfit_pose(dev_, d, b.map, d_poses, stride, 1, 0, d.n_part_rec, d_rec_atoms, (size_t)d.n_part_rec, d_base_box, d_base_row, d_overflow, stream_), "emfit_pose launch");
        hip_check(launch_emfit_list(b.map, b.table.reach, d_base_box, 1, d_items, d_n_items, stream_), "emfit_list launch");
        b.n_atoms = d.n_part_rec;
        b.atoms = d_rec_atoms;
        b.atom_stride = (size_t)d.n_part_rec;
        b.brick_sums = d_base_sums;
        b.rows = d_base_row;
        b.grid = d_base;
        hip_check(launch_emfit_bricks(b, groups(1), stream_), "emfit_bricks launch");
        b.brick_sums = nullptr;
        b.base = d_base;
        b.base_sums = d_base_sums;
    }
    b.n_atoms = count;
    b.atoms = d_atoms;
    b.atom_stride = (size_t)std::max(count, 1);
    b.rows = d_rows;
    b.grid = d_grid;
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = std::min(chunk, n - i0);
        hip_check(hipMemsetAsync(d_n_items, 0, sizeof(uint32_t), stream_), "hipMemset");
        hip_check(launch_emfit_init(d_rows, d_boxes, rigid ? d_base_row : nullptr, m, stream_), "emfit_init launch");
        if (grid) hip_check(launch_emfit_fill(d_grid, d_base, m, N, stream_), "emfit_fill launch");
        hip_check(launch_emfit_pose(dev_, d, b.map, d_poses + i0 * stride, stride, m, first, count, d_atoms, b.atom_stride, d_boxes, d_rows, d_overflow, stream_), "emfit_pose launch");
        hip_check(launch_emfit_list(b.map, b.table.reach, d_boxes, m, d_items, d_n_items, stream_), "emfit_list launch");
        hip_check(launch_emfit_bricks(b, groups(m), stream_), "emfit_bricks launch");
        hip_check(hipMemcpyAsync(h_rows.data() + i0, d_rows, m * sizeof(ld_density_sums), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H sums");
        if (grid) hip_check(hipMemcpyAsync(h_grid.data() + i0 * N, d_grid, m * N * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H voxels");
    }
    const char *message = "a simulated voxel reaches 2^24 or a pose's sum 2^40, or a posed coordinate lies beyond +-1.0e6 A";
    finish_timed(d_overflow, "density fit", message);
    // below the two limits ss < 2^24 x s < 2^64 and se <= 32767 x s < 2^55: no sum has wrapped
    for (size_t i = 0; i < n; i++)
        if (h_rows[i].s >= kEmfitSumLimit) throw Error(LD_ERR_INVALID, message);
    if (out) std::copy(h_rows.begin(), h_rows.end(), out);
    if (grid) std::copy(h_grid.begin(), h_grid.end(), grid);
}

}  // namespace ld
