// rtd_let.hpp — dose-averaged LET beside the dose path (rtd_set_let_table, rtd_field_water_depth, rtd_field_let_influence,
// rtd_let_average, rtd_optimizer_set_let_objective; include/rtd.h). Nothing here is launched by a compute, a
// transfer, a gradient or rtd_field_dose_influence, and nothing here writes what they read.
//
// The convention is the analytical one: the LET of spot j at voxel v is the LET of the spot's energy at the voxel's water-equivalent
// depth along the field. Three rules, each float32 in the stated order (-ffp-contract=off), restated in tests/let_reference.py:
//   position   the fan index k_transfer samples the BEV dose at for the voxel (TransferParams::init / getFanIdx of the state record),
//              moved into the indices of the [S][H][W] trace arrays: i = x - 32, j = y - 32 (the BEV padding), k = z + beamFirstInside;
//   depth      of trace sample (k, j, i): 0.5f * (wepl[k] + old), old = wepl[k - 1] for k > beamFirstInside and 0 otherwise — the
//              mid-point 0.5f * (cumulSp + cumulSpOld) at which k_fill deposits the step's dose (its walk starts with cumulSpOld = 0 at
//              beamFirstInside). Trilinear over the 8 samples around the position, lerpW along x, then y, then z; per axis a position
//              that is not >= 0 takes node 0 and one >= n - 1 node n - 1, both with weight 0 (CLAMP at all six faces: a voxel behind
//              the last step takes the last depth);
//   table      L(l, d): rows floor(energyIdx) and the next, clamped, with k_fill's row weight; within a row the position
//              d * energyScaleFact clamped to [0, nSamples - 1] (a NaN to 0), lerpW between floor and the next node.
// Kernels:
//   k_let_depth          one lane per voxel of a box, lanes along x, a wave per (y, z) row of the box (the divisions are per row);
//   k_let_values_csc     block j: N = D * L for the entries of column j of the CSC matrix (one layer per column);
//   k_let_values_rows    kDijApGroup lanes per row of the row-major companion (one depth per row): the same expression;
//   k_let_average        LETd = let_dose / dose above a dose floor;
//   k_let_add            the optimiser's gradient a + b, and its three objective values.
#pragma once

namespace rtd {

// Per axis of the clamped trilinear sample: the two nodes and the weight of the second.
__device__ inline void letNodes(float p, int n, int& i0, int& i1, float& a) {
    if (!(p >= 0.0f)) { i0 = 0; i1 = 0; a = 0.0f; return; }
    if (p >= (float)(n - 1)) { i0 = n - 1; i1 = n - 1; a = 0.0f; return; }
    const float fl = floorf(p);
    i0 = (int)fl; i1 = i0 + 1; a = p - fl;                           // (0 <= i0 < n - 1)
}

__device__ inline float letStepDepth(const float* __restrict__ wepl, size_t R, int first, int k, int ray) {
    const float cur = wepl[(size_t)k * R + ray];
    const float old = (k > first && k > 0) ? wepl[(size_t)(k - 1) * R + ray] : 0.0f;
    return 0.5f * (cur + old);
}

// Water-equivalent depth of the voxels of a box. useStateBox: the field's dose box of the state record (what rtd_field_clear_dose
// clears), else `box`. compact: out is indexed by the box row (x fastest inside the box), else by the voxel of the dose grid.
__global__ __launch_bounds__(256) void k_let_depth(const float* __restrict__ wepl, const FieldState* __restrict__ st, FieldConst fc, int nx, int ny,
                                                   DijBox box, int useStateBox, int compact, float* __restrict__ out) {
    if (useStateBox) {
        if (st->tboxMax[0] < st->tboxMin[0] || st->tboxMax[1] < st->tboxMin[1] || st->tboxMax[2] < st->tboxMin[2]) return;
        box = DijBox{st->tboxMin[0], st->tboxMin[1], st->tboxMin[2], st->tboxMax[0] - st->tboxMin[0] + 1, st->tboxMax[1] - st->tboxMin[1] + 1,
                     st->tboxMax[2] - st->tboxMin[2] + 1};
    }
    const int first = st->beamFirstInside;
    const TransferParams p0 = st->transfer;
    const size_t R = (size_t)fc.W * fc.H;
    const int lane = threadIdx.x % 64;
    const long long nLines = (long long)box.bh * box.bd;
    for (long long line = (long long)blockIdx.x * 4 + threadIdx.x / 64; line < nLines; line += (long long)gridDim.x * 4) {
        const int y = box.y0 + (int)(line % box.bh), z = box.z0 + (int)(line / box.bh);
        float* dst = compact ? out + line * box.bw : out + ((size_t)z * ny + y) * nx + box.x0;
        for (int dx = lane; dx < box.bw; dx += 64) {
            TransferParams p = p0;
            p.init(box.x0 + dx, y);
            const Vec3 pos = p.getFanIdx(z);
            int i0, i1, j0, j1, k0, k1; float ax, ay, az;
            letNodes(pos.x - (float)kMaxSuperpR, fc.W, i0, i1, ax);
            letNodes(pos.y - (float)kMaxSuperpR, fc.H, j0, j1, ay);
            letNodes(pos.z + (float)first, fc.S, k0, k1, az);
            const int r00 = j0 * fc.W + i0, r10 = j0 * fc.W + i1, r01 = j1 * fc.W + i0, r11 = j1 * fc.W + i1;
            const float c00 = lerpW(ax, letStepDepth(wepl, R, first, k0, r00), letStepDepth(wepl, R, first, k0, r10));
            const float c10 = lerpW(ax, letStepDepth(wepl, R, first, k0, r01), letStepDepth(wepl, R, first, k0, r11));
            const float c01 = lerpW(ax, letStepDepth(wepl, R, first, k1, r00), letStepDepth(wepl, R, first, k1, r10));
            const float c11 = lerpW(ax, letStepDepth(wepl, R, first, k1, r01), letStepDepth(wepl, R, first, k1, r11));
            dst[dx] = lerpW(az, lerpW(ay, c00, c10), lerpW(ay, c01, c11));
        }
    }
}

// A layer's part of the table lookup: the two rows and the row weight as k_fill takes them for the cumulative IDD, and the sample scale.
struct LetLayer { int row0, row1; float rowW, scale; };
__device__ inline LetLayer letLayer(const LayerPlan& lp, int nEnergies) {
    LetLayer q;
    const float py = lp.energyIdx, fy = floorf(py);
    q.rowW = py - fy; q.row0 = (int)fy; q.row1 = q.row0 + 1;
    if (!(py >= 0.0f)) { q.row0 = 0; q.row1 = 0; q.rowW = 0.0f; }
    q.row0 = q.row0 > nEnergies - 1 ? nEnergies - 1 : q.row0;
    q.row1 = q.row1 > nEnergies - 1 ? nEnergies - 1 : q.row1;
    q.scale = lp.energyScaleFact;
    return q;
}
__device__ inline float letLookup(const float* __restrict__ table, int nSamples, const LetLayer& q, float depth) {
    int x0, x1; float ax;
    letNodes(depth * q.scale, nSamples, x0, x1, ax);
    const float* r0 = table + (size_t)q.row0 * nSamples;
    const float* r1 = table + (size_t)q.row1 * nSamples;
    return lerpW(q.rowW, lerpW(ax, r0[x0], r0[x1]), lerpW(ax, r1[x0], r1[x1]));
}
// The layers' records into LDS (L <= kMaxLayers): every block of the two value kernels.
__device__ inline void letLoadLayers(const LayerPlan* __restrict__ layers, int L, int nEnergies, LetLayer* __restrict__ sh) {
    for (int l = threadIdx.x; l < L; l += blockDim.x) sh[l] = letLayer(layers[l], nEnergies);
    __syncthreads();
}

// Block j: out[e] = float32(vals[e] * L(layer of column j, depth of row rows[e])) over column j. depth is indexed by the box row.
__global__ __launch_bounds__(256) void k_let_values_csc(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                        const float* __restrict__ depth, int nx, int ny, DijBox box, const LayerPlan* __restrict__ layers,
                                                        int L, int spotsPerLayer, const float* __restrict__ table, int nEnergies, int nSamples,
                                                        float* __restrict__ out) {
    __shared__ LetLayer sLayer[kMaxLayers];
    letLoadLayers(layers, L, nEnergies, sLayer);
    const int j = blockIdx.x;
    const LetLayer q = sLayer[j / spotsPerLayer];
    const long long a = colPtr[j], b = colPtr[j + 1];
    for (long long e = a + threadIdx.x; e < b; e += blockDim.x)
        out[e] = vals[e] * letLookup(table, nSamples, q, depth[dijBoxRow(rows[e], nx, ny, box)]);
}

// kDijApGroup lanes per box row r: out[i] = float32(cVals[i] * L(layer of column cCols[i], depth[r])) over the row's entries.
__global__ __launch_bounds__(256) void k_let_values_rows(const long long* __restrict__ rowPtr, const int* __restrict__ cCols, const float* __restrict__ cVals,
                                                         const float* __restrict__ depth, long long nRows, const LayerPlan* __restrict__ layers, int L,
                                                         int spotsPerLayer, const float* __restrict__ table, int nEnergies, int nSamples,
                                                         float* __restrict__ out) {
    __shared__ LetLayer sLayer[kMaxLayers];
    letLoadLayers(layers, L, nEnergies, sLayer);
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kDijApGroup;
    const int t = threadIdx.x % kDijApGroup;
    if (r >= nRows) return;
    const long long a = rowPtr[r], b = rowPtr[r + 1];
    if (a == b) return;
    const float d = depth[r];
    for (long long i = a + t; i < b; i += kDijApGroup) out[i] = cVals[i] * letLookup(table, nSamples, sLayer[cCols[i] / spotsPerLayer], d);
}

// out[v] = dose[v] > floor ? letDose[v] / dose[v] : 0 (an IEEE division). In place on either input: a voxel is read before it is written.
__global__ __launch_bounds__(256) void k_let_average(const float* letDose, const float* dose, size_t n, float doseFloor, float* out) {
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
        const float d = dose[v], l = letDose[v];
        out[v] = d > doseFloor ? l / d : 0.0f;
    }
}

// The optimiser with a LET objective: grad = float32(grad + gradLet) per entry, and by thread 0 values3 = [f_dose + f_let, f_dose, f_let]
// with values[0] = values3[0] (float64), which k_opt_step reads.
__global__ __launch_bounds__(256) void k_let_add(float* __restrict__ grad, const float* __restrict__ gradLet, int n, double* __restrict__ values,
                                                 const double* __restrict__ valuesLet, double* __restrict__ values3) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) grad[j] = grad[j] + gradLet[j];
    if (j == 0) {
        const double fd = values[0], fl = valuesLet[0], f = fd + fl;
        values3[0] = f; values3[1] = fd; values3[2] = fl;
        values[0] = f;
    }
}

}  // namespace rtd
