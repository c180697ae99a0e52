// The selection functions behind mnerf_debug_launch_plan (api.cpp), each defined next to the launch that calls the same rule:
// conv.hip, conv_backward.hip (two), instance_norm.hip, window_attention.hip.  Host only: no device call, no launch.
#pragma once
#include <stdint.h>

int mnerf_plan_conv2d(const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);
int mnerf_plan_conv_gemm(const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);
int mnerf_plan_conv_wgrad(const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);
int mnerf_plan_instance_norm(const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);
int mnerf_plan_window_attention(const int64_t* args, int32_t n_args, int32_t* plan, int32_t n_plan);
