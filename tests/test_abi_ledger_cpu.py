"""Ledger of the C ABI: every `stil_*` entry point of include/stil_hip.h names the test function(s) that check it directly
("file::function"), or carries a short reason why it has none.  A new entry point without an entry fails here; so does an
entry whose test was renamed away.  DESIGN.md section 2 prints this table (python tests/test_abi_ledger_cpu.py)."""
import ast
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.dirname(os.path.abspath(__file__))

MAX_REASONS = 12

EP = "test_gpu_entry_points.py"
OPS = "test_gpu_ops.py"
CPU = "test_product_cpu.py"
_DEFER = f"{OPS}::test_deferred_gradient_reductions_equal_the_immediate_ones_bit_for_bit"
_BN_STATS = f"{OPS}::test_bn_statistics_two_pass_and_tile_paths_agree_with_float64"
_BN_BWD = f"{OPS}::test_gemm_epilogue_batchnorm_backward_sums"
_PLAN = f"{OPS}::test_weight_layout_plan_equals_the_per_call_layouts_bit_for_bit"
_POLICY = f"{CPU}::test_small_batch_policies_host_side"
_INFO = f"{EP}::test_size_queries_and_library_info"
_AUG = "test_gpu_augment.py"
_ALB = "test_gpu_augment_alb.py"
_AK = "test_gpu_augment_kernels.py"
_AK_CPU = "test_augment_cases_cpu.py"
_MATCH = "test_gpu_match.py"
_MK = "test_gpu_match_kernels.py"
_MK_CPU = "test_match_cases_cpu.py"
_MET = "test_gpu_metrics.py"
_METK = "test_gpu_metric_kernels.py"
_METK_CPU = "test_metric_cases_cpu.py"
_ATT = "test_gpu_attention.py"
_ATT_CPU = "test_attention_config_cpu.py"
KE = "test_gpu_kernel_edges.py"
_GEMM = "test_gpu_gemm.py"
_GEMM_CPU = "test_gemm_cases_cpu.py"
_GEMM_NT = f"{_GEMM}::test_gemm_nt_instantiations_against_float64"
_GEMM_WG = f"{_GEMM}::test_wgrad_instantiations_against_float64"
_GEMM_CODES = f"{_GEMM_CPU}::test_every_case_reports_the_code_its_table_names"
_GEMM_SPLITS = f"{_GEMM_CPU}::test_splits_slabs_and_panels_are_what_the_cases_claim"
_TAB = "test_gpu_tabular.py"
_TAB_REFUSE = "test_tabular_cases_cpu.py::test_argument_checks_refuse_before_any_launch"
_TAB_OWN = f"{_TAB}::test_each_forward_stays_inside_its_own_tokens"

# name -> list of "file::function" (checked directly there) | str (the reason it has no test of its own)
LEDGER = {
    "stil_last_error": [_INFO],
    "stil_version": [_INFO, f"{CPU}::test_library_exports_every_declared_symbol"],
    "stil_device_count": [_INFO],
    "stil_gemm_nt": [_GEMM_NT, f"{_GEMM}::test_documented_exact_relations_hold_bit_for_bit", f"{_GEMM_CPU}::test_argument_checks_refuse_before_any_launch",
                     f"{OPS}::test_gemm_nt_plain", f"{OPS}::test_conv_fwd_dgrad_wgrad", f"{OPS}::test_gemm_nt_wide_epilogue_is_the_scalar_one_bit_for_bit"],
    "stil_gemm_nt_split_workspace_bytes": [_GEMM_SPLITS, _GEMM_NT, f"{OPS}::test_gemm_split_k_is_the_unsplit_product_and_deterministic"],
    "stil_gemm_nt_force_splits": [_GEMM_SPLITS, _GEMM_NT, _POLICY],
    "stil_gemm_nt_bstats_ok": "eligibility predicate of the bstats epilogue (no arithmetic); the launches it admits are compared in "
                              "test_gemm_epilogue_batchnorm_backward_sums",
    "stil_gemm_nt_tile_rows": [_BN_STATS, f"{CPU}::test_gemm_tune_policy_and_precision_flag_arithmetic"],
    "stil_gemm_nt_variant": [f"{CPU}::test_c_abi_rejects_bad_arguments_without_a_gpu", f"{CPU}::test_gemm_tune_policy_and_precision_flag_arithmetic"],
    "stil_gemm_nt_config": [_GEMM_CODES, _GEMM_NT],
    "stil_gemm_nt_panel": [_GEMM_SPLITS],
    "stil_wgrad_workspace_bytes": [_INFO],
    "stil_wgrad_tn": [_GEMM_WG, f"{_GEMM_CPU}::test_argument_checks_refuse_before_any_launch", f"{OPS}::test_conv_fwd_dgrad_wgrad", _DEFER],
    "stil_wgrad_config": [_GEMM_CODES, _GEMM_WG],
    "stil_reduce_job_bytes": [_POLICY],
    "stil_wgrad_splits": [_POLICY, _INFO],
    "stil_wgrad_force_splits": [_GEMM_SPLITS, _GEMM_WG, _POLICY],
    "stil_wgrad_tn_partial": [_GEMM_WG, _DEFER],
    "stil_colsum_chunks": [_INFO, _POLICY],
    "stil_colsum_partial": [_DEFER],
    "stil_reduce_jobs": [_DEFER, "test_gpu_graph_step.py::test_deferred_reduce_duplicate_slot_at_low_offset"],
    "stil_colsum_workspace_bytes": [_INFO],
    "stil_colsum": [f"{EP}::test_colsum", f"{EP}::test_queue_mean_is_colsum_bit_for_bit_and_the_float64_mean"],
    "stil_conv_weight_layout": [f"{OPS}::test_conv_fwd_dgrad_wgrad", _PLAN],
    "stil_conv_weight_layout_phase": [f"{OPS}::test_strided_dgrad_phase_decomposition", _PLAN],
    "stil_weight_layouts": [_PLAN],
    "stil_weight_layout_job_bytes": [_PLAN],
    "stil_weight_layout_job_blocks": [_PLAN],
    "stil_im2col_nchw": [f"{OPS}::test_stem_and_maxpool", f"{KE}::test_im2col_nchw_equals_unfold"],
    "stil_transpose": [_PLAN, f"{KE}::test_transpose_equals_t"],
    "stil_bn_workspace_bytes": [_BN_STATS],
    "stil_bn_train_fwd": [_BN_STATS, f"{OPS}::test_conv_bn_act_train_and_eval"],
    "stil_bn_train_fwd_tiles": [_BN_STATS, f"{OPS}::test_deferred_batchnorm_is_the_materialised_path_bit_for_bit"],
    "stil_bn_tiles_workspace_bytes": [_BN_STATS],
    "stil_bn_eval_affine": [f"{EP}::test_bn_eval_affine"],
    "stil_bn_train_bwd": [_BN_BWD, f"{OPS}::test_conv_bn_act_train_and_eval", "test_gpu_bnprior.py::test_scalar_backward_final_against_float64"],
    "stil_bn_bwd_tiles_workspace_bytes": [_BN_BWD],
    "stil_bn_train_bwd_tiles": [_BN_BWD],
    "stil_maxpool3x3s2_fwd": [f"{OPS}::test_stem_and_maxpool", f"{OPS}::test_maxpool_ties_after_relu", f"{KE}::test_maxpool_ties_nan_and_all_minus_inf_windows_route_like_aten"],
    "stil_maxpool3x3s2_bwd": [f"{OPS}::test_stem_and_maxpool", f"{OPS}::test_maxpool_ties_after_relu", f"{KE}::test_maxpool_ties_nan_and_all_minus_inf_windows_route_like_aten"],
    "stil_layernorm_fwd": [f"{OPS}::test_layernorm", f"{KE}::test_layernorm_vector_kernels", f"{KE}::test_layernorm_scalar_kernels_by_shape", f"{KE}::test_layernorm_both_instantiations_on_the_same_rows"],
    "stil_layernorm_bwd_workspace_bytes": [f"{KE}::test_layernorm_bwd_refuses_before_any_write", f"{KE}::test_layernorm_vector_kernels"],
    "stil_layernorm_bwd": [f"{OPS}::test_layernorm", f"{KE}::test_layernorm_vector_kernels", f"{KE}::test_layernorm_scalar_kernels_by_shape", f"{KE}::test_layernorm_both_instantiations_on_the_same_rows", f"{KE}::test_layernorm_bwd_refuses_before_any_write"],
    "stil_attention_fwd": [f"{_ATT}::test_attention_kernels_against_float64", f"{_ATT}::test_every_kernel_is_reached_in_every_orientation",
                           f"{OPS}::test_attention"],
    "stil_attention_bwd": [f"{_ATT}::test_attention_kernels_against_float64", f"{_ATT}::test_refused_backward_launches_nothing",
                           f"{OPS}::test_attention"],
    "stil_attention_config": [f"{_ATT_CPU}::test_the_cases_of_the_gpu_test_map_to_their_kernels",
                              f"{_ATT_CPU}::test_config_is_negative_exactly_where_the_entry_points_refuse",
                              f"{_ATT_CPU}::test_the_shapes_forward_takes_and_backward_refuses_are_pinned"],
    "stil_act_bwd": [f"{EP}::test_act_bwd"],
    "stil_drop_add": [f"{EP}::test_drop_add_both_paths_all_operand_combinations", f"{EP}::test_drop_add_vector_and_scalar_paths_agree_bit_for_bit",
                      f"{EP}::test_drop_add_backward"],
    "stil_axpby": [f"{EP}::test_axpby_and_scale_dev"],
    "stil_rng_mask": [f"{OPS}::test_rng_mask_rate_and_determinism", f"{KE}::test_rng_mask_equals_the_integer_model_byte_for_byte", f"{KE}::test_rng_mask_offset_continues_the_stream"],
    "stil_counter_inc": [f"{OPS}::test_rng_mask_rate_and_determinism", f"{KE}::test_rng_mask_equals_the_integer_model_byte_for_byte"],
    "stil_tab_embed_fwd": [f"{_TAB}::test_tab_embed_against_float64", _TAB_REFUSE, f"{OPS}::test_tab_embed"],
    "stil_tab_embed_bwd_workspace_bytes": [_INFO, f"{_TAB}::test_tab_embed_against_float64", _TAB_REFUSE],
    "stil_tab_embed_bwd": [f"{_TAB}::test_tab_embed_against_float64", _TAB_REFUSE, f"{OPS}::test_tab_embed"],
    "stil_tokmean_fwd": [f"{EP}::test_tokmean"],
    "stil_tokmean_bwd": [f"{EP}::test_tokmean"],
    "stil_saint_embed_fwd": [f"{_TAB}::test_saint_embed_against_float64", _TAB_OWN, _TAB_REFUSE, f"{OPS}::test_saint_pieces"],
    "stil_saint_embed_bwd": [f"{_TAB}::test_saint_embed_against_float64", _TAB_REFUSE, f"{OPS}::test_saint_pieces"],
    "stil_colmlp_fwd": [f"{_TAB}::test_colmlp_against_float64", f"{_TAB}::test_colmlp_follows_its_pointer_tables", _TAB_OWN, _TAB_REFUSE,
                        f"{OPS}::test_saint_pieces"],
    "stil_colmlp_bwd": [f"{_TAB}::test_colmlp_against_float64", f"{_TAB}::test_colmlp_follows_its_pointer_tables", _TAB_REFUSE,
                        f"{OPS}::test_saint_pieces"],
    "stil_geglu_fwd": [f"{EP}::test_geglu"],
    "stil_geglu_bwd": [f"{EP}::test_geglu"],
    "stil_row_softmax_fwd": [f"{EP}::test_row_softmax"],
    "stil_row_softmax_bwd": [f"{EP}::test_row_softmax"],
    "stil_ce_hard": [f"{EP}::test_ce_hard", f"{OPS}::test_small_losses"],
    "stil_ce_soft": [f"{EP}::test_ce_soft", f"{OPS}::test_small_losses"],
    "stil_reduce_sum": [f"{EP}::test_reduce_sum"],
    "stil_scale_dev": [f"{EP}::test_axpby_and_scale_dev"],
    "stil_l2norm_fwd": [f"{EP}::test_l2norm"],
    "stil_l2norm_bwd": [f"{EP}::test_l2norm"],
    "stil_clip_fwd": [f"{OPS}::test_clip_and_club", f"{KE}::test_clip_fwd_bwd_on_a_logit_matrix"],
    "stil_clip_bwd": [f"{OPS}::test_clip_and_club", f"{KE}::test_clip_fwd_bwd_on_a_logit_matrix"],
    "stil_club_fwd": [f"{OPS}::test_clip_and_club", f"{KE}::test_club_against_the_materialised_form"],
    "stil_club_bwd": [f"{OPS}::test_clip_and_club", f"{KE}::test_club_against_the_materialised_form"],
    "stil_cgpl_pgls": [f"{OPS}::test_cgpl_pgls_and_prototypes", f"{OPS}::test_cgpl_top1_is_argmax_of_softmax_with_first_index_ties", f"{KE}::test_cgpl_pgls_at_every_width"],
    "stil_da_apply": [f"{EP}::test_da_apply"],
    "stil_proto_loss": [f"{EP}::test_proto_loss", f"{EP}::test_proto_loss_at_its_lds_bound"],
    "stil_proto_accum": [f"{OPS}::test_cgpl_pgls_and_prototypes", f"{KE}::test_proto_accum"],
    "stil_proto_add": [f"{EP}::test_proto_add_and_commit"],
    "stil_proto_commit": [f"{EP}::test_proto_add_and_commit"],
    "stil_contrast_graph": [f"{_MATCH}::test_contrast_graph_and_unfold_kernels_against_torch", f"{_MK}::test_contrast_graph_against_float64",
                            f"{_MK}::test_contrast_graph_row_without_an_edge_gives_zero", f"{_MK}::test_contrast_graph_fn_scales_by_the_upstream_gradient",
                            f"{_MK_CPU}::test_fp32_aten_meets_the_contrast_checks", f"{_MK_CPU}::test_contrast_graph_refuses_before_any_launch"],
    "stil_simmatch_unfold": [f"{_MATCH}::test_contrast_graph_and_unfold_kernels_against_torch", f"{_MK}::test_simmatch_unfold_against_float64",
                             f"{_MK_CPU}::test_fp32_aten_meets_the_unfold_checks", f"{_MK_CPU}::test_simmatch_unfold_refuses_before_any_launch"],
    "stil_freematch_update": [f"{_MATCH}::test_freematch_kernels_against_torch", f"{_MK}::test_freematch_update_two_calls_against_float64",
                              f"{_MK_CPU}::test_fp32_aten_meets_the_update_checks_and_rows_are_unambiguous",
                              f"{_MK_CPU}::test_freematch_update_refuses_before_any_launch"],
    "stil_freematch_entropy": [f"{_MATCH}::test_freematch_kernels_against_torch", f"{_MK}::test_freematch_entropy_against_float64",
                               f"{_MK}::test_freematch_entropy_fn_scales_by_the_upstream_gradient", f"{_MK_CPU}::test_fp32_aten_meets_the_entropy_checks",
                               f"{_MK_CPU}::test_freematch_entropy_refuses_before_any_launch"],
    "stil_flag_ratios": [f"{EP}::test_flag_ratios"],
    "stil_onehot_argmax": [f"{OPS}::test_onehot_argmax_first_maximum_and_threshold", f"{KE}::test_onehot_argmax_beyond_one_wave", f"{KE}::test_onehot_argmax_ties_across_and_within_lanes_and_at_the_threshold"],
    "stil_ema_update": [f"{OPS}::test_ema_and_adam_slabs", f"{KE}::test_ema_update_is_bit_exact_past_the_grid_cap", f"{KE}::test_ema_update_on_a_sub_slab"],
    "stil_ema_int_trunc": [f"{EP}::test_ema_int_trunc"],
    "stil_adam_step": [f"{OPS}::test_ema_and_adam_slabs", f"{KE}::test_adam_five_steps_with_padding_and_a_lagging_tensor", f"{KE}::test_adam_slab_beyond_the_grid_cap"],
    "stil_metric_topk": [f"{EP}::test_metric_topk_on_a_column_slice_and_k_edges", f"{_MET}::test_topk_accuracy_counts",
                         f"{_METK}::test_topk_counters_equal_the_sorted_position", f"{_METK}::test_topk_nan_rows_one_by_one",
                         f"{_METK}::test_counters_add_over_calls_and_an_empty_call_leaves_them",
                         f"{_METK_CPU}::test_top1_reference_is_atens_argmax_nan_rows_included"],
    "stil_metric_binary": [f"{EP}::test_metric_binary_at_the_threshold", f"{_MET}::test_binary_accuracy_and_auroc_with_ties",
                           f"{_METK}::test_binary_counters_equal_the_comparison", f"{_METK}::test_counters_add_over_calls_and_an_empty_call_leaves_them",
                           f"{_METK_CPU}::test_binary_reference_is_atens_comparison"],
    "stil_auroc_workspace_bytes": [f"{EP}::test_auroc_single_row_and_all_scores_equal", f"{_METK}::test_auroc_workspace_bound_and_refusals"],
    "stil_auroc": [f"{EP}::test_auroc_single_row_and_all_scores_equal", f"{_MET}::test_multiclass_auroc", f"{_MET}::test_binary_accuracy_and_auroc_with_ties",
                   f"{_METK}::test_auroc_equals_the_pair_count_bit_for_bit", f"{_METK}::test_auroc_workspace_bound_and_refusals",
                   f"{_METK}::test_auroc_nan_in_one_column_leaves_the_other_classes_alone",
                   f"{_METK}::test_two_rank_metrics_equal_one_process_on_the_concatenation", f"{_METK_CPU}::test_auroc_reference_against_sklearn"],
    "stil_tab_corrupt": [f"{_AUG}::test_tab_corrupt_matches_reference_golden_bit_for_bit", f"{_AK}::test_tab_corrupt_copies_and_scatters_exactly",
                         f"{_AK_CPU}::test_tab_corrupt_refuses_before_any_launch"],
    "stil_tab_corrupt_draw": [f"{EP}::test_tab_corrupt_draw", f"{EP}::test_tab_corrupt_draw_rejects_more_than_8192_columns",
                              f"{_AUG}::test_tab_corrupt_device_draws_are_valid_and_uniform"],
    "stil_aug_gray_mean": [f"{_AUG}::test_colour_jitter_matches_torchvision_float_formulas", f"{_AK}::test_gray_mean_against_float64",
                           f"{_AK_CPU}::test_gray_mean_refuses_before_any_launch"],
    "stil_aug_blur": [f"{_AUG}::test_gaussian_blur_matches_torchvision_formula", f"{_AK}::test_blur_against_float64",
                      f"{_AK_CPU}::test_blur_refuses_before_any_launch"],
    "stil_aug_rotate": [f"{_AUG}::test_rotate_matches_bilinear_reflect101_restatement", f"{_AK}::test_rotate_against_float64",
                        f"{_AK_CPU}::test_rotate_refuses_before_any_launch"],
    "stil_aug_hue": [f"{_AUG}::test_hue_matches_torchvision_float_formulas", f"{_AK}::test_hue_against_float64", f"{_AK_CPU}::test_hue_refuses_before_any_launch"],
    "stil_aug_resize": [f"{_AUG}::test_resize_crop_flip_matches_interpolate", f"{_AUG}::test_colour_jitter_matches_torchvision_float_formulas",
                        f"{_AK}::test_resize_crop_flip_against_float64", f"{_AK}::test_resize_colour_jitter_against_float64",
                        f"{_AK}::test_resize_clamps_bad_device_boxes_into_the_image", f"{_AK_CPU}::test_resize_refuses_before_any_launch"],
    "stil_alb_color": [f"{_ALB}::test_color_u8_brightness_contrast_all_orders_bit_exact", f"{_ALB}::test_color_full_chain_with_hue_saturation_gray",
                       f"{_AK}::test_alb_color_at_the_pixel_count_edges_and_in_place",
                       f"{_AK}::test_alb_color_and_to_tensor_from_a_misaligned_base_take_the_per_pixel_path",
                       f"{_AK}::test_alb_color_with_64_workgroups_per_image"],
    "stil_alb_blur": [f"{_ALB}::test_blur_reflect101_borders", f"{_AK}::test_alb_blur_at_the_tile_edges",
                      f"{_AK}::test_alb_blur_on_images_shorter_than_the_radius"],
    "stil_alb_resize": [f"{_ALB}::test_resize_crop_flip_and_to_tensor", f"{_AK}::test_alb_resize_of_one_pixel_wide_sources_both_outputs"],
    "stil_alb_rotate": [f"{_ALB}::test_rotate_quantised_reflect101", f"{_AK}::test_alb_rotate_of_narrow_images_with_and_without_flip_first"],
    "stil_alb_to_tensor": [f"{_ALB}::test_resize_crop_flip_and_to_tensor", f"{_AK}::test_alb_to_tensor_at_the_pixel_count_edges",
                           f"{_AK}::test_alb_color_and_to_tensor_from_a_misaligned_base_take_the_per_pixel_path"],
    "stil_ring_enqueue": [f"{EP}::test_ring_enqueue_matches_python_ring", f"{EP}::test_ring_enqueue_rejects_bad_arguments_before_any_write"],
    "stil_queue_mean": [f"{EP}::test_queue_mean_is_colsum_bit_for_bit_and_the_float64_mean", f"{EP}::test_queue_mean_clamps_the_count"],
    "stil_rows_append": [f"{EP}::test_rows_append_matches_python_store",
                         f"{EP}::test_auroc_reserved_store_equals_the_list_mode_and_raises_after_overflow"],
}


def _test_functions(filename):
    """names of the module-level test functions of tests/<filename>, read with ast (the GPU modules are not imported)"""
    with open(os.path.join(TESTS, filename)) as f:
        tree = ast.parse(f.read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_every_entry_point_is_in_the_ledger():
    from stil_tta_amd._lib import parse_header
    header = set(parse_header())
    assert header == set(LEDGER), f"not in the ledger: {sorted(header - set(LEDGER))}; not in the header: {sorted(set(LEDGER) - header)}"


def test_every_named_test_exists():
    cache = {}
    for name, entry in LEDGER.items():
        if isinstance(entry, str):
            assert len(entry) > 20, f"{name}: a reason, not a shrug"
            continue
        assert entry, f"{name}: no test named"
        for ref in entry:
            fname, func = ref.split("::")
            if fname not in cache:
                cache[fname] = _test_functions(fname)
            assert func in cache[fname], f"{name}: {ref} does not exist"


def test_few_entry_points_go_without_a_test():
    reasons = sorted(n for n, e in LEDGER.items() if isinstance(e, str))
    assert len(reasons) <= MAX_REASONS, reasons


def test_design_md_prints_this_ledger():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert markdown_table() in f.read(), "DESIGN.md section 2: regenerate the table (python tests/test_abi_ledger_cpu.py)"


def markdown_table():
    rows = ["| entry point | direct test (tests/) or reason |", "|---|---|"]
    for name, entry in LEDGER.items():
        cell = f"none: {entry}" if isinstance(entry, str) else ", ".join(f"`{e}`" for e in entry)
        rows.append(f"| `{name}` | {cell} |")
    return "\n".join(rows)


if __name__ == "__main__":
    print(markdown_table())
