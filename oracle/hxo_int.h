/* hxo_int.h - ORACLE internals (test infrastructure). */
#ifndef HXO_INT_H
#define HXO_INT_H
#include "hxo.h"

#define HXO_MAX(a, b) ((a) > (b) ? (a) : (b))
#define HXO_MIN(a, b) ((a) < (b) ? (a) : (b))

float hxo_bits2f(uint32_t u);
uint32_t hxo_f2bits(float f);
void hxo_math_init(void);
int hxo_round(float x);
int hxo_logsubber(int n1, int n2);
float hxo_dblog(float x);
int hxo_dual_g(float x);
float hxo_anwin(int n);
extern float hxo_quant_off[32];

int hxo_huff_dim(int t);
int hxo_huff_linbits(int t);
int hxo_huff_code(int t, int x, int y);
int hxo_huff_len(int t, int x, int y);
int hxo_quada_code(int v);
int hxo_quada_len(int v);

int hxo_sfb_long_edge(int sr_index, int i);
int hxo_sfb_short_edge(int sr_index, int i);
int hxo_sfbl_limit(int sr_index, int band_limit);
int hxo_sfbs_limit(int sr_index, int band_limit);
int hxo_nearest_sf_band_freq(int tix, int samprate, int freq);
int hxo_samprate_mpeg1(int sr_index);
void hxo_init_transform_tables(hxo_params *p);
void hxo_init_psy_long(hxo_params *p);
void hxo_init_psy_short(hxo_params *p);
void hxo_count_init(void);

/* short-block allocator (hxo_short.c) */
int hxo_ms_metric_short(hxo_encoder *e, const float x[2][576]);
int hxo_bitallo_short(hxo_encoder *e, float xr[2][576], hxo_sigmask sm[2][36],
                      int min_bits, int target_bits, int max_bits, int bit_pool,
                      hxo_scalefact sf_out[2], hxo_gr gr[2], int ms_flag, int MNR);
void hxo_short_init(hxo_encoder *e);

/* first-generation allocator (hxo_alloc1.c) */
void hxo_a1_init(hxo_encoder *e);
int hxo_a1_ms_metric(hxo_encoder *e, const float x[2][576]);
void hxo_bitallo1(hxo_encoder *e, float xr[][576], hxo_sigmask sm[][36], int ch_arg, int nchan_arg,
                  int min_bits, int target_bits, int max_bits, hxo_scalefact sf_out[], hxo_gr gr[],
                  int ix[][576], unsigned char signx[][576], int ms_flag);
int hxo_pack_sf_lsf_is(hxo_bitw *w, hxo_scalefact *sf, int nsf_stereo);

/* Path census (tests/alloc_path_cases.py, tools/alloc_path_search.py): how often each branch of the rate control, the
   Huffman pick and the frame driver was taken, over every encoder of the process.  Not part of the encoder: nothing reads
   the counts back.  One name per line; oracle/oracle.py lists the same names in the same order.
   L_ long allocator, S_ short allocator, A_ first-generation allocator, H_ Huffman pick (per coded channel-granule; H_tab0 ..
   H_tab31 follow the last name: a region of at least one pair coded with that table, whichever of the three regions),
   D_ frame driver.  The H_ entries are counted where a granule's Huffman data is packed, so a granule coded as nothing
   (no call of hxo_pack_huff) counts nowhere: H_no_bigv is a packed granule that has count1 quadruples only. */
#define HXO_PATHS(X) \
    X(L_inc_ms) X(L_inc_lr) X(L_inc_hf) X(L_inc_first) X(L_inc_several) X(L_inc_cap) X(L_inc_gmin_hold) X(L_inc_stepback) \
    X(L_dec_ms) X(L_dec_lr) X(L_dec_one) X(L_dec_several) X(L_dec_cap) X(L_dec_delta_floor) X(L_dec_delta_formula) \
    X(L_dec_after_stepback) X(L_lim_max) X(L_lim_max_several) X(L_lim_p23_one) X(L_lim_p23_both) X(L_lim_after_dec_cap) \
    X(L_isf2_refined) X(L_isf2_clamp_up) X(L_isf2_clamp_lo) \
    X(L_fb_dmnr_raised) X(L_fb_dmnr_cut) X(L_fb_mnr_cap) X(L_fb_reset) \
    X(L_bt1_adjust) X(L_bt3_adjust) X(L_short_mnr0_cbr) X(L_short_mnr0_vbr) \
    X(S_inc_enter) X(S_inc_first) X(S_inc_several) X(S_inc_cap) X(S_dec_enter) X(S_dec_first) X(S_dec_several) X(S_dec_cap) \
    X(S_lim_enter) X(S_lim_first) X(S_lim_several) X(S_lim_cap) X(S_p23_enter) X(S_p23_first) X(S_p23_several) X(S_p23_cap) \
    X(S_mnr_raise) X(S_only_over_skip) \
    X(A_seek1_dsf0) X(A_seek1_dsf2) X(A_seek1_four) X(A_seek2_dsf0) X(A_seek2_dsf2) X(A_seek2_four) X(A_minbits_corr) \
    X(A_more_enter) X(A_more_gz) X(A_more_three) X(A_back_enter) X(A_back_several) X(A_back_gg100) \
    X(H_count1_a) X(H_count1_b) X(H_escape) X(H_bigv_limit) X(H_empty_region) X(H_no_bigv) \
    X(D_pool_cap_stuffing) X(D_cbr_padding_slot) X(D_vbr_ibr_min) X(D_vbr_ibr_max) X(D_vbr_pool_step) X(D_vbr_limit_cut) \
    X(D_ms_frame) X(D_lr_frame) X(D_scfsi_shared) X(D_no_frame_out) X(D_two_frames_out) X(D_lsf_bitmin_40) \
    X(D_lsf_vbr_span10) X(D_lsf_vbr_span16) X(D_lsf_vbr_span25)
#define HXO_PATH_ENUM(n) HXO_P_##n,
enum { HXO_PATHS(HXO_PATH_ENUM) HXO_P_H_tab0, HXO_P_N = HXO_P_H_tab0 + 32 };
extern long long hxo_path_counts[HXO_P_N];
#define HXO_HIT(n) (hxo_path_counts[HXO_P_##n]++)
#endif
