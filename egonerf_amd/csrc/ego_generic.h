// Internal (not part of the C ABI): the any-shape compatibility kernels of ego_generic.hip / ego_generic_march.hip, called by the ABI
// entry points of ego_pack.hip / ego_shade.hip / ego_march.hip when the scene's shape is not the tuned one.
#pragma once
#include "../../include/egonerf_hip.h"

bool ego_shape_is_tuned(const ego_scene* sc);   // app_dim 27, 48 appearance components, MLP_Fea 150 -> 128 -> 128 -> 3 with view_pe = fea_pe = 2
int64_t ego_generic_packed_floats(const ego_scene* sc);
int ego_generic_pack(const ego_scene* sc, float* out, void* stream);
int ego_generic_shade(const ego_scene* sc, const float* rays, const float* coords, int64_t N, int32_t S, float* rgb, const uint8_t* tile_active,
                      void* stream);
int ego_generic_app_feature(const ego_scene* sc, const float* c7n, int64_t M, float* out, void* stream);
int ego_generic_mlp_fea(const ego_scene* sc, const float* viewdirs, const float* feat, int64_t M, float* rgb, void* stream);
struct MarchArgs;   // csrc/ego_march.h
int ego_generic_march(const MarchArgs& a, void* stream);
// the envelope of the any-shape kernels (ego_generic.hip, over the shared checks of ego_host.h; asked by all three sources): EGO_OK or the refusal
int check_generic_shape(const ego_scene* sc, const char* who, bool need_tables, bool need_mlp, bool need_packed = true);
