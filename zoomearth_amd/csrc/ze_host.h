// Host-side declarations shared by the engine translation units.
#pragma once
#include <stdint.h>

#include <vector>

struct ze_coeffs {
    int ksize = 0, out_size = 0, max_cnt = 0;
    std::vector<int> xmin, xcnt, kk;
};
void ze_bicubic_coeffs(int in_size, int out_size, ze_coeffs* c);
int ze_smart_resize_impl(int height, int width, int factor, int64_t min_pixels, int64_t max_pixels, int* out_h,
                         int* out_w);
void ze_window_index_impl(const int32_t* grid_thw, int n_images, int merge, int window_size, int patch,
                          std::vector<int64_t>& window_index, std::vector<int32_t>& cu_window);
void ze_vision_pos_ids_impl(const int32_t* grid_thw, int n_images, int merge, std::vector<int32_t>& hw);
int ze_rope_index_impl(const int32_t* ids, int len, const int32_t* grid_thw, int n_images, int image_token_id,
                       int merge, int32_t* pos, int32_t* rope_delta);

// ---- beam search, host only (ze_index.cpp; the callers are in ze_beam.hip): argument and table checks and the divisor table, free of
// any device call so that the same source runs under -fsanitize in a stand-alone program (tests/cabi_san/ze_beam_host_san.cpp).
// Return 0, or a ze_status value (-1 invalid, -4 not found) with *why set to a static message.
int ze_beam_check_impl(const int32_t* seqs, int groups, int num_beams, int num_return_sequences, int max_new_tokens, int early_stopping,
                       float length_penalty, float repetition_penalty, int max_seqs, int max_ctx, const char** why);
int ze_kv_reorder_check_impl(const int32_t* src_seqs, const int32_t* dst_seqs, int n, int row0, int rows, int max_seqs, int max_ctx,
                             const char** why);
// divs[n] = float(max(n, 1) ** length_penalty) for n = 0 .. max_new_tokens: the divisor HF computes in Python floats
void ze_beam_divs_impl(float length_penalty, int max_new_tokens, std::vector<float>& divs);
// the groups of `live` that go on at step t: not done, and t inside their token budget
void ze_beam_live_impl(const std::vector<int>& live, const std::vector<char>& done, const std::vector<int>& budget, int t, std::vector<int>& still);
