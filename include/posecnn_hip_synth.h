/*
 * posecnn_hip_synth.h — synthetic training scenes rendered on the device: what the reference's render thread
 * (tools/train_net.py:155-258) gets from Synthesizer::render (lib/synthesize/synthesize.cpp:345-609, OpenGL) with the
 * background paste of lib/gt_synthesize_layer/minibatch.py:147-154. Same library as posecnn_hip.h, same status codes and
 * conventions, same ABI version. The arithmetic — which is this library's own, GL's is not reproducible — is written out at
 * the top of posecnn_amd/csrc/synth_scene.hip and restated in numpy by tests/synth_ref.py.
 *
 * The mesh bank (DEVICE memory, 16-byte aligned; resident across calls)
 *   vertices, normals  f32   [Nv][3]   pooled over the meshes, object frame
 *   colors             f32   [Nv][3]   RGB in [0, 1], or NULL: meshes without a texture are white
 *   uvs                f32   [Nv][2]   or NULL when no mesh is textured; v runs upwards as in Wavefront OBJ
 *   faces              int32 [Nf][3]   pooled; indices LOCAL to the mesh. A face with an index outside its mesh's
 *                                      vertex range is dropped by the kernel, never followed.
 *   textures           uint8 [texture_bytes]  pooled RGB images, row-major [height][width][3], or NULL
 * The tables (HOST memory: they are a few rows, validated and packed on the host before the device is touched)
 *   mesh_table         int32 [M][4]    (first vertex, vertex count, first face, face count); at most 2^27 faces per mesh
 *   texture_table      int32 [M][3]    (byte offset, height, width); width 0 = the mesh uses its vertex colours; NULL = none
 *   instance_ids       int32 [N][3]    (scene, mesh, class id 1..63), sorted by scene; an instance's position inside its
 *                                      scene is its slot; at most PCNN_SYNTH_MAX_INSTANCES per scene
 *   instance_params    f32   [N][13]   pose 3x4 row-major (camera <- object), shininess (an integer 1..255)
 *   lights             f32   [S][4]    (x, y, z, intensity) of the scene's point light, camera frame
 * Per call, DEVICE memory
 *   background         uint8 [S][H][W][3]  BGR, or NULL (black)
 * Outputs (DEVICE memory, every element written)
 *   color         uint8  [S][H][W][4]  BGRA; alpha 255 on a hit, 0 on a miss, where BGR is the background pixel
 *   depth         uint16 [S][H][W]     trunc(min(65535, factor_depth * z)), 0 on a miss
 *   label         int32  [S][H][W]     class id of the front-most surface, 0 on a miss
 *   vertmap       f32    [S][H][W][3]  object-frame surface point, 0 on a miss; may be NULL
 *   pixel_counts  int32  [N]           label pixels owned by each instance
 *   valid         int32  [S]           1 when every instance of the scene owns >= min_pixels pixels (an empty scene is valid)
 * num_scenes == 0 and num_instances == 0 are legal. The call enqueues a fixed sequence of kernels on `stream`; it never
 * synchronises with the host, allocates or reads a result back.
 */
#ifndef POSECNN_HIP_SYNTH_H_
#define POSECNN_HIP_SYNTH_H_

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_SYNTH_MAX_INSTANCES 32

int pcnn_synth_scene_workspace_bytes(int num_scenes, int height, int width, size_t* bytes);

int pcnn_synth_scene_fwd(const float* vertices, const float* normals, const float* colors, const float* uvs,
                         const int32_t* faces, int num_vertices, int num_faces, const int32_t* mesh_table,
                         int num_meshes, const uint8_t* textures, size_t texture_bytes, const int32_t* texture_table,
                         const int32_t* instance_ids, const float* instance_params, int num_instances,
                         const float* lights, const uint8_t* background, int num_scenes, int height, int width,
                         float fx, float fy, float px, float py, float z_near, float z_far, float factor_depth,
                         int min_pixels, uint8_t* color, uint16_t* depth, int32_t* label, float* vertmap,
                         int32_t* pixel_counts, int32_t* valid, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_HIP_SYNTH_H_ */
