// hip_stub.cpp -- TEST INFRASTRUCTURE for the sanitizer build of the host side (`make asan`).
//
// GPU AddressSanitizer is not available on this pool, so the host C++ (PDB / setup.json / npy /
// DCparams readers, docking-model builders, tile layout, scorer and GSO bookkeeping, the analysis
// half's checks, workspace sizing and PDB writer, both CLIs' error paths) is compiled with g++ -fsanitize=address,undefined and linked against THIS file
// instead of the HIP runtime and the kernels: device memory is host memory (so every upload,
// download and workspace size is checked by ASan), streams / events are no-ops, kernel launches do
// nothing, graph capture is refused (the eager path runs).  Energies are therefore meaningless in
// this build; nothing of it ships.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kernels/cluster.hpp"
#include "kernels/dfire_bm.hpp"
#include "kernels/dfire_packed.hpp"
#include "kernels/dfire_tiled.hpp"
#include "kernels/gso_step.hpp"
#include "kernels/pose_energy.hpp"
#include "lightdock_hip.h"
#include "stub_access.hpp"

extern "C" {
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *p, int) {
    std::memset(p, 0, sizeof *p);
    std::strcpy(p->gcnArchName, "gfx950:sramecc+:xnack-");
    return hipSuccess;
}
static std::vector<size_t> allocation_sizes;   // of every hipMalloc so far
size_t ld_stub_device_allocations(void) { return allocation_sizes.size(); }   // host_check: what a scorer's construction allocated
size_t ld_stub_device_allocations_of(size_t bytes) { return (size_t)std::count(allocation_sizes.begin(), allocation_sizes.end(), bytes); }   // ... in blocks of exactly that size
hipError_t hipMalloc(void **p, size_t n) { allocation_sizes.push_back(n); *p = std::malloc(n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { std::free(p); return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { std::memset(d, v, n); return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t *s) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *g) { *g = nullptr; return hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t *, hipGraph_t, hipGraphNode_t *, char *, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = nullptr; return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = nullptr; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hip stub"; }
}

namespace ld {
// kernel launch entry points: the arguments are touched, nothing runs
// touch / peek (stub_access.hpp): the first and the last element of a buffer a kernel writes / reads, the extent as the kernel indexes it
size_t pair_kernel_lds_bytes(const PairLaunch &) { return 0; }
const char *pair_kernel_name(int method) { return method == 0 ? "pose_energy_pairs<0" : "pose_energy_pairs<1"; }
static void peek_molecule(const DeviceMolecule &m, bool dfire) {
    const size_t n_pad = (size_t)m.n_pad;
    peek(m.x, n_pad);
    peek(m.y, n_pad);
    peek(m.z, n_pad);
    peek(m.slot, n_pad);
    if (dfire) {
        peek(m.tindex, n_pad);
    } else {
        peek(m.charge, n_pad);
        peek(m.well_depth, n_pad);
        peek(m.radius, n_pad);
    }
    peek(m.modes, (size_t)m.num_anm * 3 * n_pad);   // [mode][xyz][n_pad]
}
static size_t pair_kernel_launches = 0;
extern "C" size_t ld_stub_pair_kernel_launches(void) { return pair_kernel_launches; }   // host_check: which route a batch took
hipError_t launch_pair_kernel(const PairLaunch &p, hipStream_t) {
    pair_kernel_launches++;
    const bool dfire = p.method == LD_METHOD_DFIRE;
    if (p.rec.n_pad < p.rec.n || p.lig.n_pad < p.lig.n || p.n_chunks * p.chunk_atoms < p.rec.n) return hipErrorInvalidValue;
    peek_molecule(p.rec, dfire);
    peek_molecule(p.lig, dfire);
    if (dfire) {
        peek(p.table, (size_t)LD_DFIRE_TABLE_LEN);
        peek(p.lut, (size_t)kDfireLutCells);
        peek(p.bin_step, (size_t)kDfireSteps);
    }
    if (!p.n_poses) return hipSuccess;
    peek(p.poses, (p.n_poses - 1) * p.stride + 7 + (p.use_anm ? (size_t)(p.rec.num_anm + p.lig.num_anm) : 0));   // row i: poses + i * stride
    if (p.active) peek(p.active, p.n_poses);
    touch(p.partial, p.n_poses * (size_t)p.n_chunks * 2);                            // [pose][chunk][2]
    touch(p.flags, p.n_poses * (size_t)(p.rec.flag_words + p.lig.flag_words));     // [pose][rec words + lig words]
    if (p.count_partial) touch(p.count_partial, p.n_poses * (size_t)p.n_chunks);   // [pose][chunk]
    return hipSuccess;
}
hipError_t launch_finish_kernel(const FinishLaunch &f, hipStream_t) {
    for (size_t i = 0; i < f.n_poses; i++)
        if (!f.active || f.active[i]) f.energies[i] = 0.0;   // the output buffer really has n_poses doubles
    return hipSuccess;
}
size_t packed_kernel_lds_bytes(int) { return 0; }
hipError_t launch_dfire_packed(const PackedLaunch &t, hipStream_t) {
    if (t.n_poses && t.partial) t.partial[2 * (t.n_poses * (size_t)t.n_groups - 1) + 1] = 0.0;   // last slot of the workspace
    return hipSuccess;
}
size_t bm_pairs_lds_bytes() { return 0; }
// The block-major launches write the first and the last element of EVERY workspace region of the launch's set, indexed from the
// BmLaunch fields the way the kernels index them (kernels/dfire_bm.hpp: the comments of BmLaunch) -- not through bm_layout(), so
// that ASan checks the layout's offsets and sizes independently.  Rows of the pass run to t.cap, the room a set has.
hipError_t launch_bm_pose(const BmLaunch &t, hipStream_t) {
    if (!t.n_poses) return hipSuccess;
    const size_t tile_pairs = (size_t)t.m.lig.n_tiles * t.m.rec_n_tiles;
    const size_t flag_words = (size_t)(t.m.rec_flag_words + t.m.lig.flag_words);
    touch(t.rt, 12 * t.cap);
    touch(t.rt_exact, 8 * t.cap);
    touch(t.tp_count, tile_pairs + kBmCounters + kBmCullQueueWords);   // the sequence's counters lie behind the tile pairs' counts
    touch(t.tile_sum, t.cap * (size_t)t.m.lig.n_tiles);
    touch(t.exact_fix, t.cap);
    if (flag_words) touch(t.flags + t.first * flag_words, t.n_poses * flag_words);
    if (t.m.anm_rec + t.m.anm_lig > 0) {
        touch(t.amp, t.cap * kBmAmpFloats);
        touch(t.amp_exact, t.cap * 2 * kBmMaxModes);
        touch(t.anm_sub, t.cap * (size_t)t.m.rec_n_tiles * 8);   // dfire_bm_rec_boxes
        touch(t.anm_tile, t.cap * (size_t)t.m.rec_n_tiles);
    }
    if (t.count_mode) {
        touch(t.tile_tested, t.cap * (size_t)t.m.lig.n_tiles);
        touch(t.exact_pairs, t.cap);
    }
    return hipSuccess;
}
hipError_t launch_bm_cull(const BmLaunch &t, hipStream_t) {
    if (!t.n_poses) return hipSuccess;
    const size_t tile_pairs = (size_t)t.m.lig.n_tiles * t.m.rec_n_tiles;
    touch(t.ent_row, tile_pairs * t.cap);
    touch(t.ent_mask, tile_pairs * t.cap);
    touch(t.job_count, (size_t)kBmCounters + kBmCullQueueWords);   // the culling kernel's item counters: job_count + kBmCounters + queue
    if (t.job_next != t.job_count + 1) return hipErrorInvalidValue;
    return hipSuccess;
}
hipError_t launch_bm_pairs(const BmLaunch &t, hipStream_t) {
    if (!t.n_poses) return hipSuccess;
    const size_t tile_pairs = (size_t)t.m.lig.n_tiles * t.m.rec_n_tiles;
    const size_t parts = tile_pairs * (t.cap / 64 + 1), waves = (size_t)t.pairs_groups * kBmWavesPerCu;
    touch(t.jobs, parts * 2);                     // dfire_bm_plan
    touch(t.job_cost, parts * kBmJobRows);        // dfire_bm_census
    touch(t.job_rec, parts * kBmJobRows * 4);
    touch(t.job_order, parts * kBmJobRows);       // dfire_bm_order
    touch(t.job_next, 1);
    touch(t.ent_partial, waves * kBmPartEntries);   // [wave][kBmPartEntries]
    touch(t.queue, waves * kBmQueueCap);
    // a job loads its part's entries without looking at the part's end: a read of up to one part behind the last tile pair's list
    volatile uint32_t row = t.ent_row[tile_pairs * t.cap + kBmPartEntries - 1];
    volatile unsigned long long mask = t.ent_mask[tile_pairs * t.cap + kBmPartEntries - 1];
    (void)row;
    (void)mask;
    if (t.debug) touch(t.debug, waves * kBmDebugWords);
    return hipSuccess;
}
hipError_t launch_bm_gather(const BmLaunch &t, hipStream_t) {
    if (t.n_poses && !t.count_mode) touch(t.partial + 2 * t.first, 2 * t.n_poses);
    if (t.n_poses && t.count_mode) {
        touch(t.count_partial + t.first, t.n_poses);
        touch(t.tested_partial + t.first, t.n_poses);
        touch(t.exact_partial + t.first, t.n_poses);
    }
    return hipSuccess;
}
// The analysis launches (kernels/cluster.hpp) likewise: the first and the last element of every buffer a kernel reads or writes,
// the extents from the launch arguments as the kernels of cluster.hip index them, not from complex.cpp's sizing.
hipError_t launch_complex_pose_xyz(const ComplexDevice &m, const double *poses, size_t stride, size_t n, double *out, hipStream_t) {
    peek_complex(m, poses, stride, n);
    std::memset(out, 0, n * (size_t)(m.n_rec + m.n_lig) * 3 * sizeof(double));   // ld_complex_write_pdb prints these
    return hipSuccess;
}
hipError_t launch_complex_pose_thousandths(const ComplexDevice &m, const double *poses, size_t stride, int n_swarms, int G,
                                           const uint32_t *backbone, int n_bb, int32_t *ws, int *overflow, hipStream_t) {
    peek_complex(m, poses, stride, (size_t)n_swarms * G);   // row s * G + g
    peek(backbone, (size_t)n_bb);
    touch(ws, (size_t)n_swarms * n_bb * 3 * G);             // ws[((s * n_bb + b) * 3 + c) * G + g]
    peek(overflow, 1);                                      // set, never cleared, by the kernel
    return hipSuccess;
}
hipError_t launch_complex_bsas(const int32_t *ws, const double *scoring, int n_swarms, int G, int n_bb, double, int32_t *cluster_of,
                               int32_t *representatives, uint32_t *n_clusters, hipStream_t) {
    if (G < 1 || G > kMaxGlowworms) return hipErrorInvalidValue;   // the sort keys' LDS
    peek(ws, (size_t)n_swarms * n_bb * 3 * G);
    peek(scoring, (size_t)n_swarms * G);
    // cleared whole: what the call returns is then the same whatever the block held before (history_check compares it)
    std::memset(cluster_of, 0, (size_t)n_swarms * G * sizeof(int32_t));
    std::memset(representatives, 0, (size_t)n_swarms * G * sizeof(int32_t));
    std::memset(n_clusters, 0, (size_t)n_swarms * sizeof(uint32_t));
    return hipSuccess;
}
hipError_t launch_complex_contacts(const ComplexDevice &m, const ContactsDevice &d, const double *poses, size_t stride, size_t n, uint32_t,
                                   size_t slots, int4 *atoms_ws, int *boxes_ws, uint32_t *rec_bits, uint32_t *lig_bits, int *overflow,
                                   hipStream_t) {
    const size_t rw = ((size_t)d.n_rec_res + 31) >> 5, lw = ((size_t)d.n_lig_res + 31) >> 5;
    const size_t n_boxes = (size_t)d.n_rec_res + d.n_lig_res + d.n_lig_grp;
    if (slots < 1 || slots > (size_t)kContactSlots) return hipErrorInvalidValue;
    if ((rw + lw) * sizeof(uint32_t) + (d.boxes_in_lds ? n_boxes * 6 * sizeof(int) : 0) > 160 * 1024) return hipErrorInvalidValue;   // a CU's LDS
    peek_complex(m, poses, stride, n);
    peek(d.res_start, (size_t)d.n_rec_res + d.n_lig_res + 1);
    peek(d.res_of_atom, (size_t)d.n_atoms);
    touch(atoms_ws, slots * d.n_atoms);                               // atoms_ws + blockIdx * n_atoms
    if (!d.boxes_in_lds) touch(boxes_ws, slots * 6 * n_boxes);        // boxes_ws + blockIdx * 6 * n_boxes
    std::memset(rec_bits, 0, n * rw * sizeof(uint32_t));              // cleared whole, as launch_complex_bsas's outputs are
    std::memset(lig_bits, 0, n * lw * sizeof(uint32_t));
    peek(overflow, 1);
    return hipSuccess;
}
static size_t packed_prepare_launches = 0;
extern "C" size_t ld_stub_packed_prepare_launches(void) { return packed_prepare_launches; }   // host_check: what a scorer's construction launched
hipError_t launch_packed_prepare(const PackedPrepareLaunch &p, hipStream_t) {
    packed_prepare_launches++;
    if (p.n_poses && p.pairs_out) std::memset(p.pairs_out, 0, p.n_poses * (size_t)p.n_tiles * 32 * sizeof(PackedRecPair));
    if (p.n_poses && p.sub_out) std::memset(p.sub_out, 0, p.n_poses * (size_t)p.n_tiles * 8 * sizeof(TiledBox));
    if (p.n_poses && p.tile_out) std::memset(p.tile_out, 0, p.n_poses * (size_t)p.n_tiles * sizeof(TiledBox));
    return hipSuccess;
}
size_t gso_kernel_lds_bytes(const GsoLaunch &) { return 0; }
hipError_t launch_gso_step(const GsoLaunch &g, hipStream_t) {
    const size_t total = (size_t)g.n_swarms * g.n_glowworms;
    std::memcpy(g.poses_out, g.poses_in, total * g.pose_len * sizeof(double));   // both pose buffers are that large
    for (size_t i = 0; i < total; i++) g.step[i]++;
    return hipSuccess;
}
}  // namespace ld
