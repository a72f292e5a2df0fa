// The two rotation conversions of the validation loss (loss.hip) as device functions.  rotmat_to_aa_dev IS the body of thmr_op_rotmat_to_aa's
// kernel (tokenizer.hip calls it: contraction is off inside it, and the kernel's instructions are the same ones as before the move).
// aa_to_rotmat_dev restates the body of head.hip's aa_to_rotmat_kernel line for line (TWIN: change both together); that kernel keeps its
// own copy, because its contraction is left to the compiler, calling this function from it changes how the compiler packs the same
// operations (v_pk_mul_f32 / v_pk_fma_f32), and its bits are pinned by tests.  tests/test_gpu_val_loss.py holds the two together: the
// loss of an axis-angle ground truth against the loss of thmr_op_aa_to_rotmat's matrices of it.
#pragma once
#include <hip/hip_runtime.h>

// aa_to_rotmat (tokenhmr/lib/utils/geometry.py:5-44): axis-angle -> quaternion -> rotation matrix, operation by operation
// (angle = ||theta + 1e-8||, axis = theta / angle, half-angle quaternion, re-normalised, nine quadratic forms); R row-major
__device__ __forceinline__ void aa_to_rotmat_dev(float tx, float ty, float tz, float* R) {
    const float ex = tx + 1e-8f, ey = ty + 1e-8f, ez = tz + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float nx = tx / angle, ny = ty / angle, nz = tz / angle;
    const float half = angle * 0.5f;
    const float qw = cosf(half), sn = sinf(half);
    const float qx = sn * nx, qy = sn * ny, qz = sn * nz;
    const float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    const float w = qw / qn, x = qx / qn, y = qy / qn, z = qz / qn;
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;    R[2] = 2 * wy + 2 * xz;
    R[3] = 2 * wz + 2 * xy;    R[4] = w2 - x2 + y2 - z2; R[5] = 2 * yz - 2 * wx;
    R[6] = 2 * xz - 2 * wy;    R[7] = 2 * wx + 2 * yz;    R[8] = w2 - x2 - y2 + z2;
}

// matrix_to_quaternion (rotation_utils.py:104-163) + quaternion_to_axis_angle (:478-506) of one row-major matrix.  Every value the
// reference computes for the winning candidate is computed here by the same fp32 operations in the same order; contraction into FMAs is off.
__device__ __forceinline__ void rotmat_to_aa_dev(const float* __restrict__ m, float& ax, float& ay, float& az) {
#pragma clang fp contract(off)
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    // _sqrt_positive_part of the four squared magnitudes (:122-132)
    const float s[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    float qa[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) qa[k] = s[k] > 0.f ? sqrtf(s[k]) : 0.f;
    // q_abs.argmax(dim=-1), lowest index on ties (:161-163)
    int w = 0;
    float best = qa[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (qa[k] > best) { best = qa[k]; w = k; }
    // the winning row of quat_by_rijk (:135-151) over 2 max(q_abs, 0.1) (:155-156; safe_zero_division's clamp at the smallest normal
    // number never bites a denominator >= 0.2)
    float q0, q1, q2, q3;
    const float sq = best * best;
    if (w == 0)      { q0 = sq;        q1 = m21 - m12; q2 = m02 - m20; q3 = m10 - m01; }
    else if (w == 1) { q0 = m21 - m12; q1 = sq;        q2 = m10 + m01; q3 = m02 + m20; }
    else if (w == 2) { q0 = m02 - m20; q1 = m10 + m01; q2 = sq;        q3 = m12 + m21; }
    else             { q0 = m10 - m01; q1 = m20 + m02; q2 = m21 + m12; q3 = sq; }
    const float den = 2.0f * fmaxf(best, 0.1f);
    q0 = q0 / den; q1 = q1 / den; q2 = q2 / den; q3 = q3 / den;
    // quaternion_to_axis_angle (:492-506)
    const float norm = sqrtf(q1 * q1 + q2 * q2 + q3 * q3);
    const float half = atan2f(norm, q0);
    const float angle = 2.0f * half;
    const float so = fabsf(angle) < 1e-6f ? 0.5f - (angle * angle) / 48.0f : sinf(half) / angle;
    const float d = fmaxf(so, 1.17549435e-38f);        // safe_zero_division: clamp(min = finfo(float32).tiny)
    ax = q1 / d;
    ay = q2 / d;
    az = q3 / d;
}
