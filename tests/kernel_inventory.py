"""Which test launches which kernel on its own: every __global__ function of csrc/*.hip and csrc/*.h, mapped to (test file, the entry point or
public function named in that file through which the test reaches the kernel without a whole model forward around it), or to
("forward only", reason).  tests/test_kernel_inventory_host.py keeps the table equal to the sources.  The "forward only" entries are the
agenda for later per-kernel tests."""

FORWARD_ONLY = "forward only"

_ROWS, _TOKENS, _EPI, _GEMM = "test_gpu_rows.py", "test_gpu_tokens.py", "test_gpu_gemm_epi.py", "test_gpu_gemm.py"
_CRERANK, _QUERY, _CLUSTER, _RELATED = "test_gpu_crerank.py", "test_gpu_query.py", "test_gpu_cluster.py", "test_gpu_related.py"

KERNEL_TESTS = {
    # attention
    "attn_kernel": ("test_gpu_attention.py", "hiptsdbg_attention_run"),
    "attn2_kernel": ("test_gpu_attention_exact.py", "hiptsdbg_attention2_launch"),
    "attn3_kernel": ("test_gpu_attention_exact.py", "hiptsdbg_attention2_launch"),
    "swin_attn_kernel": ("test_gpu_swinv2.py", "hiptsdbg_swinv2_window_attention"),
    # GEMM main loops (HIPTS_GEMM selects the older ones per process) and epilogues
    "gemm_pp_kernel": (_EPI, "hiptsdbg_gemm_epilogue"),
    "gemm_dw_kernel": (_GEMM, "hiptsdbg_gemm_run"),
    "gemm_pp2_kernel": (_GEMM, "hiptsdbg_gemm_run"),
    "gemm_s3_kernel": (_GEMM, "hiptsdbg_gemm_run"),
    "gemm_kernel": (_GEMM, "hiptsdbg_gemm_run"),
    "gemm_q4_kernel": (_GEMM, "hiptsdbg_gemm_q4_compare"),
    "gelu_probe_kernel": (_GEMM, "hiptsdbg_gelu"),
    # rows, stems, folded LayerNorm
    "row_ln_kernel": (_ROWS, "hiptsdbg_row_ln"),
    "pool_ln_kernel": (_ROWS, "hiptsdbg_pool_ln"),
    "patch_gather_kernel": (_ROWS, "hiptsdbg_patch_gather"),
    "patchify_u8_kernel": (_ROWS, "hiptsdbg_patch_gather"),
    "patchify_u8_p16_kernel": (_ROWS, "hiptsdbg_vit_patchify_u8_p16"),
    "stem_im2col_u8_kernel": (_ROWS, "hiptsdbg_ccip_stem_u8"),
    "rowstat_kernel": ("test_gpu_ln_fold.py", "hiptsdbg_rowstat"),
    "fold_ln_kernel": ("test_gpu_ln_fold.py", "hiptsdbg_fold_ln"),
    # the small kernels at the head and tail of the forwards
    "pool_partial_kernel": (_TOKENS, "hiptsdbg_vit_pool"),
    "pool_finalize_kernel": (_TOKENS, "hiptsdbg_vit_pool"),
    "eva_assemble_kernel": (_TOKENS, "hiptsdbg_eva_assemble"),
    "eva_colsum_kernel": (_TOKENS, "hiptsdbg_eva_colsum"),
    "sw_merge_kernel": (_TOKENS, "hiptsdbg_swinv2_merge"),
    "sw_split_x_kernel": (_TOKENS, "hiptsdbg_swinv2_split_x"),
    "sw_mean_kernel": (_TOKENS, "hiptsdbg_swinv2_mean"),
    "ds_im2col_kernel": (_TOKENS, "hiptsdbg_ccip_ds_im2col"),
    "cnx_cast_kernel": (_TOKENS, "hiptsdbg_convnext_cast"),
    # convolution blocks
    "dwconv7_kernel": ("test_gpu_ccip.py", "hiptsdbg_dwconv7"),
    "dwconv7_mfma_kernel": ("test_gpu_ccip.py", "hiptsdbg_dwconv7"),
    "mlp_fused_kernel": ("test_gpu_ccip.py", "hiptsdbg_mlp_fused"),
    # character features
    "unit_rows_kernel": (FORWARD_ONLY, "behind hipts_ccip_metric, which test_gpu_flows.py calls on whole feature sets against the oracle's differences: no case "
                                       "isolates the normalisation from the Gram differences"),
    "gram_diff_kernel": (FORWARD_ONLY, "behind hipts_ccip_metric with unit_rows_kernel in front of it: the same flow test, no tile-edge or exact-answer case of its own"),
    "crerank_filter_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_offsets_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_compact_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_sort_small_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_radix_hist_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_radix_scan_kernel": (_CRERANK, "hipts_crerank_run"),
    "crerank_radix_scatter_kernel": (_CRERANK, "hipts_crerank_run"),
    "radius_pairs_kernel": (_CLUSTER, "radius_neighbors"),
    "radius_scan_kernel": (_CLUSTER, "radius_neighbors"),
    "radius_sort_rows_kernel": (_CLUSTER, "radius_neighbors"),
    "radius_core_kernel": (_CLUSTER, "cluster"),
    "radius_sweep_kernel": (_CLUSTER, "cluster"),
    "radius_roots_kernel": (_CLUSTER, "cluster"),
    "radius_assign_kernel": (_CLUSTER, "cluster"),
    "hamming_pairs_kernel": ("test_gpu_hamming.py", "hipts_radius_create_hamming"),
    # Doc2Vec and tag selection
    "d2v_infer_kernel": ("test_gpu_d2v_tags.py", "infer_batch"),
    "d2v_infer_plan_kernel": ("test_gpu_d2v_tags.py", "infer_batch"),
    "d2v_lane_major_kernel": ("test_gpu_d2v_tags.py", "Doc2VecInference"),
    "d2v_infer_dm_kernel": ("test_gpu_d2v_tags.py", "infer_batch"),
    "d2v_train_kernel": ("test_gpu_d2v_train.py", "hipts_d2v_train"),
    "tagsel_kernel": ("test_gpu_d2v_tags.py", "TagSelector"),
    # images
    "imghash_bins_kernel": ("test_gpu_imghash.py", "hipts_image_hash_u8"),
    "imghash_finish_kernel": ("test_gpu_imghash.py", "hipts_image_hash_u8"),
    "jpeg_idct_kernel": ("test_gpu_jpeg.py", "hipts_jpeg_decode_rgb"),
    "jpeg_rgb_kernel": ("test_gpu_jpeg.py", "hipts_jpeg_decode_rgb"),
    "jpeg_idct_batch_kernel": ("test_gpu_jpeg.py", "hipts_jpeg_batch_u8"),
    "jpeg_rgb_batch_kernel": ("test_gpu_jpeg.py", "hipts_jpeg_batch_u8"),
    "jpeg_encode_kernel": ("test_gpu_jpegenc.py", "hipts_jpeg_encode_batch_u8"),
    "png_unfilter_kernel": ("test_gpu_png.py", "hipts_png_decode_rgb"),
    "resample_h_kernel": ("test_gpu_resize.py", "hipts_resize_u8"),
    "resample_v_kernel": ("test_gpu_resize.py", "hipts_resize_u8"),
    "resample_h_pad_kernel": (FORWARD_ONLY, "no launch site in csrc: resample_h_pad_batch_kernel does its work for every caller; nothing can run it until something launches it"),
    "resample_h_pad_batch_kernel": ("test_gpu_jpeg.py", "hipts_resize_batch_u8"),
    "resample_v_batch_kernel": ("test_gpu_jpeg.py", "hipts_resize_batch_u8"),
    "synth_images_kernel": (FORWARD_ONLY, "hipts_synth_images_u8 makes the benchmark's and test_gpu_multirank.py's input images; its bytes are compared with nothing but themselves"),
    # query path
    "bm25_score_kernel": (_QUERY, "score"),
    "bm25_postings_kernel": (_QUERY, "score"),
    "bm25_postings_sliced_kernel": (_QUERY, "score"),
    "bm25_max_reduce_kernel": (_QUERY, "score"),
    "rowmax_kernel": (_QUERY, "score_topk"),
    "combine_kernel": (_QUERY, "score_topk"),
    "sim_mfma_kernel": (_QUERY, "query"),
    "sim_mfma_wide_kernel": (_QUERY, "query"),
    "sim1_kernel": (_QUERY, "query"),
    "retile_kernel": (_QUERY, "add_matrix"),
    "search1_score_kernel": (_QUERY, "hipts_search"),
    "search1_combine_kernel": (_QUERY, "hipts_search"),
    "search1_collect_kernel": (_QUERY, "hipts_search"),
    "search1_finish_kernel": (_QUERY, "hipts_search"),
    "mask_ranked_before_kernel": (_QUERY, "hipts_topk_after"),
    "topk_kernel": ("test_gpu_topk_arms.py", "hipts_topk"),
    "related_count_kernel": (_RELATED, "hipts_bm25_related"),
    "related_score_kernel": (_RELATED, "hipts_bm25_related"),
    "related_finish_kernel": (_RELATED, "hipts_bm25_related"),
    "rerank_finish_kernel": ("test_gpu_find_similar_batch.py", "hipts_rerank_finish"),
}
