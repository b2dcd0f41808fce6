/* libicn: entry points added since the icn.h freeze at ABI 9.
 *
 * include/icn.h is held to a fixed set of prototypes (tests/test_abi.py); what the library has gained since is declared here,
 * exported from the same libicn.so under the same conventions: plain device pointers and ints, the caller owns every buffer, the
 * library allocates nothing and never synchronises, an int entry returns 0 on success and a negative value with icn_last_error()
 * otherwise, and arguments are checked before any device call.  ICN_ABI_VERSION stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.SIGNATURES_EXT (checked against this header by tests/test_abi_ext.py). */
#ifndef ICN_EXT_H
#define ICN_EXT_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Normal agreement of two sampled surfaces: for sample s of mesh pair b, the face fa = face_a[b,s] of mesh a (vertices va (B, Va, 3),
 * faces_a (Fa, 3) shared by the batch) against the face fb = face_b[b,s] of mesh b -- the face a surface sample lies on
 * (icn_mesh_sample_fwd) and the closest face of the other mesh (icn_point_to_mesh), in either order.  Per face (i0, i1, i2):
 *   e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 in fp32 with every product of the cross product rounded on its own (a face with two
 *   coincident vertices has n exactly 0);  the normal is RESOLVED iff |n|^2 2^22 > |e1|^2 |e2|^2 and all of that is finite (the
 *   sine of the angle at vertex 0 above 1 / 2048: the rule of icn_point_to_mesh);  n^ = n / |n| where resolved.
 *   c = n^_a . n^_b;   t[b,s] = 1 - c if oriented != 0, else 1 - |c|.
 * An unresolved face on either side gives t = 1 and a zero gradient on both sides.  A face id outside [0, F), and a face with a
 * vertex id outside [0, V), count as unresolved; nothing is read out of bounds.  Non-finite vertices leave the normal unresolved:
 * t = 1, never NaN.
 * face_a / face_b (B, S) int32, t (B, S).  One launch on `stream`, no workspace, no reduction (the caller takes the mean): a pure
 * function of its inputs.  B <= 65535 per call (the batch index is gridDim.y), 2 S must fit an int. */
int icn_face_normal_agree_fwd(const float* va, const int32_t* faces_a, const int32_t* face_a, int Va, int Fa,
                              const float* vb, const int32_t* faces_b, const int32_t* face_b, int Vb, int Fb,
                              int B, int S, int oriented, float* t, void* stream);

/* Backward of icn_face_normal_agree_fwd to the vertices of either mesh, from the same inputs and dt (B, S), the upstream gradient.
 * With sigma = 1 (oriented) or sign(c) (the derivative of |c| at c = 0 is taken as 0), for side a
 *   h = -sigma dt (n^_b - c n^_a) / |n_a|;   d/dv1 = e2 x h,  d/dv2 = h x e1,  d/dv0 = -(d/dv1 + d/dv2)
 * and likewise for side b.  dva (B, Va, 3) / dvb (B, Vb, 3): either may be NULL and is then not computed; one that is given is
 * written whole.  With both NULL nothing is launched and the call returns 0.  Per side two launches: a record pass (two records
 * per sample) and the vertex scatter of icn_mesh_sample_bwd over 2 S records -- summed per vertex in a fixed order (by sample, d/dv1
 * before d/dv2), no floating-point atomics: bit-identical run to run, and a vertex no sample touches gets an exact zero.  An
 * unresolved sample contributes nothing.  2 S V integer compares per mesh and side.
 * ws: icn_face_normal_agree_bwd_workspace_bytes(B, S, Va, Vb) bytes (host-only query; 40 * 2 * B * S, 0 for sizes the call rejects),
 * 16-byte aligned, owned by the caller, only looked at when dva or dvb is given; both sides use it in turn, in stream order.
 * B <= 65535 per call, 2 S must fit an int.  0 on success, negative with icn_last_error() otherwise. */
size_t icn_face_normal_agree_bwd_workspace_bytes(int B, int S, int Va, int Vb);
int icn_face_normal_agree_bwd(const float* va, const int32_t* faces_a, const int32_t* face_a, int Va, int Fa,
                              const float* vb, const int32_t* faces_b, const int32_t* face_b, int Vb, int Fb,
                              int B, int S, int oriented, const float* dt, float* dva, float* dvb, void* ws, size_t ws_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_EXT_H */
