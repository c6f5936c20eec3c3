// D=64 fp16: 176 VGPRs + 128 AGPRs in asm, LDS 69632 B
//   P1.1:  8 MFMA,  51 fillers (16 exp), filler issue  274 cyc, cap/gap 35, est. 338 cyc
//   P2.1:  8 MFMA,  42 fillers (16 exp), filler issue  240 cyc, cap/gap 30, est. 304 cyc
//   P3.1:  8 MFMA,  57 fillers (16 exp), filler issue  290 cyc, cap/gap 37, est. 354 cyc
//   P4.1:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   P1.0:  8 MFMA,  51 fillers (16 exp), filler issue  274 cyc, cap/gap 35, est. 338 cyc
//   P2.0:  8 MFMA,  42 fillers (16 exp), filler issue  240 cyc, cap/gap 30, est. 304 cyc
//   P3.0:  8 MFMA,  57 fillers (16 exp), filler issue  290 cyc, cap/gap 37, est. 354 cyc
//   P4.0:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   loop (2 tiles): 64 MFMA, 304 VALU (4.75 per MFMA), 4 nop wait states, 492 instructions
// D=64 bf16: 176 VGPRs + 128 AGPRs in asm, LDS 69632 B
//   P1.1:  8 MFMA,  56 fillers (16 exp), filler issue  294 cyc, cap/gap 37, est. 358 cyc
//   P2.1:  8 MFMA,  50 fillers (16 exp), filler issue  272 cyc, cap/gap 34, est. 336 cyc
//   P3.1:  8 MFMA,  62 fillers (16 exp), filler issue  310 cyc, cap/gap 39, est. 374 cyc
//   P4.1:  8 MFMA,  49 fillers (16 exp), filler issue  258 cyc, cap/gap 33, est. 322 cyc
//   P1.0:  8 MFMA,  56 fillers (16 exp), filler issue  294 cyc, cap/gap 37, est. 358 cyc
//   P2.0:  8 MFMA,  50 fillers (16 exp), filler issue  272 cyc, cap/gap 34, est. 336 cyc
//   P3.0:  8 MFMA,  62 fillers (16 exp), filler issue  310 cyc, cap/gap 39, est. 374 cyc
//   P4.0:  8 MFMA,  49 fillers (16 exp), filler issue  258 cyc, cap/gap 33, est. 322 cyc
//   loop (2 tiles): 64 MFMA, 356 VALU (5.56 per MFMA), 4 nop wait states, 544 instructions
// D=128 fp16: 224 VGPRs + 256 AGPRs in asm, LDS 135168 B
//   P1.1: 16 MFMA,  65 fillers (16 exp), filler issue  338 cyc, cap/gap 22, est. 512 cyc
//   P2.1: 16 MFMA,  62 fillers (16 exp), filler issue  328 cyc, cap/gap 21, est. 512 cyc
//   P3.1: 16 MFMA,  74 fillers (16 exp), filler issue  358 cyc, cap/gap 23, est. 512 cyc
//   P4.1: 16 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 16, est. 512 cyc
//   P1.0: 16 MFMA,  65 fillers (16 exp), filler issue  338 cyc, cap/gap 22, est. 512 cyc
//   P2.0: 16 MFMA,  62 fillers (16 exp), filler issue  328 cyc, cap/gap 21, est. 512 cyc
//   P3.0: 16 MFMA,  74 fillers (16 exp), filler issue  358 cyc, cap/gap 23, est. 512 cyc
//   P4.0: 16 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 16, est. 512 cyc
//   loop (2 tiles): 128 MFMA, 336 VALU (2.62 per MFMA), 4 nop wait states, 708 instructions
// D=128 bf16: 224 VGPRs + 256 AGPRs in asm, LDS 135168 B
//   P1.1: 16 MFMA,  70 fillers (16 exp), filler issue  358 cyc, cap/gap 23, est. 512 cyc
//   P2.1: 16 MFMA,  70 fillers (16 exp), filler issue  360 cyc, cap/gap 23, est. 512 cyc
//   P3.1: 16 MFMA,  79 fillers (16 exp), filler issue  378 cyc, cap/gap 24, est. 512 cyc
//   P4.1: 16 MFMA,  54 fillers (16 exp), filler issue  278 cyc, cap/gap 18, est. 512 cyc
//   P1.0: 16 MFMA,  70 fillers (16 exp), filler issue  358 cyc, cap/gap 23, est. 512 cyc
//   P2.0: 16 MFMA,  70 fillers (16 exp), filler issue  360 cyc, cap/gap 23, est. 512 cyc
//   P3.0: 16 MFMA,  79 fillers (16 exp), filler issue  378 cyc, cap/gap 24, est. 512 cyc
//   P4.0: 16 MFMA,  54 fillers (16 exp), filler issue  278 cyc, cap/gap 18, est. 512 cyc
//   loop (2 tiles): 128 MFMA, 388 VALU (3.03 per MFMA), 4 nop wait states, 760 instructions
// D=64 fp16, four chains: 192 VGPRs + 256 AGPRs in asm, LDS 139264 B
//   A0.1:  8 MFMA,  51 fillers (16 exp), filler issue  274 cyc, cap/gap 35, est. 338 cyc
//   B0.1:  8 MFMA,  38 fillers (16 exp), filler issue  224 cyc, cap/gap 28, est. 288 cyc
//   A1.1:  8 MFMA,  57 fillers (16 exp), filler issue  290 cyc, cap/gap 37, est. 354 cyc
//   B1.1:  8 MFMA,  32 fillers (16 exp), filler issue  192 cyc, cap/gap 24, est. 256 cyc
//   A2.1:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   B2.1:  8 MFMA,  33 fillers (16 exp), filler issue  194 cyc, cap/gap 25, est. 258 cyc
//   A3.1:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   B3.1:  8 MFMA,  36 fillers (16 exp), filler issue  208 cyc, cap/gap 26, est. 272 cyc
//   A0.0:  8 MFMA,  51 fillers (16 exp), filler issue  274 cyc, cap/gap 35, est. 338 cyc
//   B0.0:  8 MFMA,  38 fillers (16 exp), filler issue  224 cyc, cap/gap 28, est. 288 cyc
//   A1.0:  8 MFMA,  57 fillers (16 exp), filler issue  290 cyc, cap/gap 37, est. 354 cyc
//   B1.0:  8 MFMA,  32 fillers (16 exp), filler issue  192 cyc, cap/gap 24, est. 256 cyc
//   A2.0:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   B2.0:  8 MFMA,  33 fillers (16 exp), filler issue  194 cyc, cap/gap 25, est. 258 cyc
//   A3.0:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   B3.0:  8 MFMA,  36 fillers (16 exp), filler issue  208 cyc, cap/gap 26, est. 272 cyc
//   loop (2 tiles): 128 MFMA, 576 VALU (4.50 per MFMA), 8 nop wait states, 836 instructions
// D=64 bf16, four chains: 192 VGPRs + 256 AGPRs in asm, LDS 139264 B
//   A0.1:  8 MFMA,  56 fillers (16 exp), filler issue  294 cyc, cap/gap 37, est. 358 cyc
//   B0.1:  8 MFMA,  46 fillers (16 exp), filler issue  256 cyc, cap/gap 32, est. 320 cyc
//   A1.1:  8 MFMA,  62 fillers (16 exp), filler issue  310 cyc, cap/gap 39, est. 374 cyc
//   B1.1:  8 MFMA,  40 fillers (16 exp), filler issue  224 cyc, cap/gap 28, est. 288 cyc
//   A2.1:  8 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 31, est. 310 cyc
//   B2.1:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   A3.1:  8 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 31, est. 310 cyc
//   B3.1:  8 MFMA,  44 fillers (16 exp), filler issue  240 cyc, cap/gap 30, est. 304 cyc
//   A0.0:  8 MFMA,  56 fillers (16 exp), filler issue  294 cyc, cap/gap 37, est. 358 cyc
//   B0.0:  8 MFMA,  46 fillers (16 exp), filler issue  256 cyc, cap/gap 32, est. 320 cyc
//   A1.0:  8 MFMA,  62 fillers (16 exp), filler issue  310 cyc, cap/gap 39, est. 374 cyc
//   B1.0:  8 MFMA,  40 fillers (16 exp), filler issue  224 cyc, cap/gap 28, est. 288 cyc
//   A2.0:  8 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 31, est. 310 cyc
//   B2.0:  8 MFMA,  41 fillers (16 exp), filler issue  226 cyc, cap/gap 29, est. 290 cyc
//   A3.0:  8 MFMA,  46 fillers (16 exp), filler issue  246 cyc, cap/gap 31, est. 310 cyc
//   B3.0:  8 MFMA,  44 fillers (16 exp), filler issue  240 cyc, cap/gap 30, est. 304 cyc
//   loop (2 tiles): 128 MFMA, 680 VALU (5.31 per MFMA), 8 nop wait states, 940 instructions
// Generated by cuda-flash-attention_amd/gen/gen_fwd_hs.py -- do not edit.
// Hand-scheduled forward tile loop of fa2_fwd_hs_kernel<D> (kernel_fa2_optimized_f16.cu).
#pragma once

#define FA2_HS_ASM_D64_F16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v162, 0\n\t" \
    "v_mov_b32 v163, 0\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "ds_read_b128 a[64:67], v0 offset:0\n\t" \
    "ds_read_b128 a[68:71], v1 offset:0\n\t" \
    "ds_read_b128 a[72:75], v2 offset:0\n\t" \
    "ds_read_b128 a[76:79], v3 offset:0\n\t" \
    "ds_read_b128 a[80:83], v0 offset:4096\n\t" \
    "ds_read_b128 a[84:87], v1 offset:4096\n\t" \
    "ds_read_b128 a[88:91], v2 offset:4096\n\t" \
    "ds_read_b128 a[92:95], v3 offset:4096\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:4096\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:4096\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:4096\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[64:67], 0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[112:115], a[64:67], 0\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[96:99], a[80:83], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[112:115], a[80:83], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_max3_f32 v160, v0, v1, v2\n\t" \
    "v_max3_f32 v160, v160, v3, v4\n\t" \
    "v_max3_f32 v160, v160, v5, v6\n\t" \
    "v_max3_f32 v160, v160, v7, v8\n\t" \
    "v_max3_f32 v160, v160, v9, v10\n\t" \
    "v_max3_f32 v160, v160, v11, v12\n\t" \
    "v_max3_f32 v160, v160, v13, v14\n\t" \
    "v_max3_f32 v160, v160, v15, v16\n\t" \
    "v_max3_f32 v160, v160, v17, v18\n\t" \
    "v_max3_f32 v160, v160, v19, v20\n\t" \
    "v_max3_f32 v160, v160, v21, v22\n\t" \
    "v_max3_f32 v160, v160, v23, v24\n\t" \
    "v_max3_f32 v160, v160, v25, v26\n\t" \
    "v_max3_f32 v160, v160, v27, v28\n\t" \
    "v_max3_f32 v160, v160, v29, v30\n\t" \
    "v_max_f32 v160, v160, v31\n\t" \
    "v_mov_b32 v174, v160\n\t" \
    "v_mov_b32 v175, v160\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v174, v175\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v160, v174, v175\n\t" \
    "v_max3_f32 v161, v32, v33, v34\n\t" \
    "v_max3_f32 v161, v161, v35, v36\n\t" \
    "v_max3_f32 v161, v161, v37, v38\n\t" \
    "v_max3_f32 v161, v161, v39, v40\n\t" \
    "v_max3_f32 v161, v161, v41, v42\n\t" \
    "v_max3_f32 v161, v161, v43, v44\n\t" \
    "v_max3_f32 v161, v161, v45, v46\n\t" \
    "v_max3_f32 v161, v161, v47, v48\n\t" \
    "v_max3_f32 v161, v161, v49, v50\n\t" \
    "v_max3_f32 v161, v161, v51, v52\n\t" \
    "v_max3_f32 v161, v161, v53, v54\n\t" \
    "v_max3_f32 v161, v161, v55, v56\n\t" \
    "v_max3_f32 v161, v161, v57, v58\n\t" \
    "v_max3_f32 v161, v161, v59, v60\n\t" \
    "v_max3_f32 v161, v161, v61, v62\n\t" \
    "v_max_f32 v161, v161, v63\n\t" \
    "v_mov_b32 v174, v161\n\t" \
    "v_mov_b32 v175, v161\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v174, v175\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v161, v174, v175\n\t" \
    "v_sub_f32 v64, 0, v160\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v160\n\t" \
    "v_sub_f32 v1, v1, v160\n\t" \
    "v_sub_f32 v2, v2, v160\n\t" \
    "v_sub_f32 v3, v3, v160\n\t" \
    "v_sub_f32 v4, v4, v160\n\t" \
    "v_sub_f32 v5, v5, v160\n\t" \
    "v_sub_f32 v6, v6, v160\n\t" \
    "v_sub_f32 v7, v7, v160\n\t" \
    "v_sub_f32 v8, v8, v160\n\t" \
    "v_sub_f32 v9, v9, v160\n\t" \
    "v_sub_f32 v10, v10, v160\n\t" \
    "v_sub_f32 v11, v11, v160\n\t" \
    "v_sub_f32 v12, v12, v160\n\t" \
    "v_sub_f32 v13, v13, v160\n\t" \
    "v_sub_f32 v14, v14, v160\n\t" \
    "v_sub_f32 v15, v15, v160\n\t" \
    "v_sub_f32 v16, v16, v160\n\t" \
    "v_sub_f32 v17, v17, v160\n\t" \
    "v_sub_f32 v18, v18, v160\n\t" \
    "v_sub_f32 v19, v19, v160\n\t" \
    "v_sub_f32 v20, v20, v160\n\t" \
    "v_sub_f32 v21, v21, v160\n\t" \
    "v_sub_f32 v22, v22, v160\n\t" \
    "v_sub_f32 v23, v23, v160\n\t" \
    "v_sub_f32 v24, v24, v160\n\t" \
    "v_sub_f32 v25, v25, v160\n\t" \
    "v_sub_f32 v26, v26, v160\n\t" \
    "v_sub_f32 v27, v27, v160\n\t" \
    "v_sub_f32 v28, v28, v160\n\t" \
    "v_sub_f32 v29, v29, v160\n\t" \
    "v_sub_f32 v30, v30, v160\n\t" \
    "v_sub_f32 v31, v31, v160\n\t" \
    "v_sub_f32 v80, 0, v161\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v161\n\t" \
    "v_sub_f32 v33, v33, v161\n\t" \
    "v_sub_f32 v34, v34, v161\n\t" \
    "v_sub_f32 v35, v35, v161\n\t" \
    "v_sub_f32 v36, v36, v161\n\t" \
    "v_sub_f32 v37, v37, v161\n\t" \
    "v_sub_f32 v38, v38, v161\n\t" \
    "v_sub_f32 v39, v39, v161\n\t" \
    "v_sub_f32 v40, v40, v161\n\t" \
    "v_sub_f32 v41, v41, v161\n\t" \
    "v_sub_f32 v42, v42, v161\n\t" \
    "v_sub_f32 v43, v43, v161\n\t" \
    "v_sub_f32 v44, v44, v161\n\t" \
    "v_sub_f32 v45, v45, v161\n\t" \
    "v_sub_f32 v46, v46, v161\n\t" \
    "v_sub_f32 v47, v47, v161\n\t" \
    "v_sub_f32 v48, v48, v161\n\t" \
    "v_sub_f32 v49, v49, v161\n\t" \
    "v_sub_f32 v50, v50, v161\n\t" \
    "v_sub_f32 v51, v51, v161\n\t" \
    "v_sub_f32 v52, v52, v161\n\t" \
    "v_sub_f32 v53, v53, v161\n\t" \
    "v_sub_f32 v54, v54, v161\n\t" \
    "v_sub_f32 v55, v55, v161\n\t" \
    "v_sub_f32 v56, v56, v161\n\t" \
    "v_sub_f32 v57, v57, v161\n\t" \
    "v_sub_f32 v58, v58, v161\n\t" \
    "v_sub_f32 v59, v59, v161\n\t" \
    "v_sub_f32 v60, v60, v161\n\t" \
    "v_sub_f32 v61, v61, v161\n\t" \
    "v_sub_f32 v62, v62, v161\n\t" \
    "v_sub_f32 v63, v63, v161\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v164, v0, v1\n\t" \
    "v_pk_add_f16 v165, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v166, v8, v9\n\t" \
    "v_pk_add_f16 v167, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v164, v164, v16\n\t" \
    "v_pk_add_f16 v165, v165, v17\n\t" \
    "v_pk_add_f16 v166, v166, v18\n\t" \
    "v_pk_add_f16 v167, v167, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v164, v164, v24\n\t" \
    "v_pk_add_f16 v165, v165, v25\n\t" \
    "v_pk_add_f16 v166, v166, v26\n\t" \
    "v_pk_add_f16 v167, v167, v27\n\t" \
    "v_pk_add_f16 v164, v164, v165\n\t" \
    "v_pk_add_f16 v166, v166, v167\n\t" \
    "v_pk_add_f16 v164, v164, v166\n\t" \
    "v_cvt_f32_f16_e32 v172, v164\n\t" \
    "v_cvt_f32_f16_sdwa v174, v164 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v172, v172, v174\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v168, v32, v33\n\t" \
    "v_pk_add_f16 v169, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v170, v40, v41\n\t" \
    "v_pk_add_f16 v171, v42, v43\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:22528\n\t" \
    "v_accvgpr_write_b32 a32, 0\n\t" \
    "v_accvgpr_write_b32 a33, 0\n\t" \
    "v_accvgpr_write_b32 a34, 0\n\t" \
    "v_accvgpr_write_b32 a35, 0\n\t" \
    "v_accvgpr_write_b32 a36, 0\n\t" \
    "v_accvgpr_write_b32 a37, 0\n\t" \
    "v_accvgpr_write_b32 a38, 0\n\t" \
    "v_accvgpr_write_b32 a39, 0\n\t" \
    "v_accvgpr_write_b32 a40, 0\n\t" \
    "v_accvgpr_write_b32 a41, 0\n\t" \
    "v_accvgpr_write_b32 a42, 0\n\t" \
    "v_accvgpr_write_b32 a43, 0\n\t" \
    "v_accvgpr_write_b32 a44, 0\n\t" \
    "v_accvgpr_write_b32 a45, 0\n\t" \
    "v_accvgpr_write_b32 a46, 0\n\t" \
    "v_accvgpr_write_b32 a47, 0\n\t" \
    "v_accvgpr_write_b32 a48, 0\n\t" \
    "v_accvgpr_write_b32 a49, 0\n\t" \
    "v_accvgpr_write_b32 a50, 0\n\t" \
    "v_accvgpr_write_b32 a51, 0\n\t" \
    "v_accvgpr_write_b32 a52, 0\n\t" \
    "v_accvgpr_write_b32 a53, 0\n\t" \
    "v_accvgpr_write_b32 a54, 0\n\t" \
    "v_accvgpr_write_b32 a55, 0\n\t" \
    "v_accvgpr_write_b32 a56, 0\n\t" \
    "v_accvgpr_write_b32 a57, 0\n\t" \
    "v_accvgpr_write_b32 a58, 0\n\t" \
    "v_accvgpr_write_b32 a59, 0\n\t" \
    "v_accvgpr_write_b32 a60, 0\n\t" \
    "v_accvgpr_write_b32 a61, 0\n\t" \
    "v_accvgpr_write_b32 a62, 0\n\t" \
    "v_accvgpr_write_b32 a63, 0\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[96:99], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[112:115], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:8192\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:8192\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:8192\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:8192\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:12288\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:12288\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:12288\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:12288\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v168, v168, v48\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "v_pk_add_f16 v169, v169, v49\n\t" \
    "v_pk_add_f16 v170, v170, v50\n\t" \
    "v_pk_add_f16 v171, v171, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[112:115], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v168, v168, v56\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_pk_add_f16 v169, v169, v57\n\t" \
    "v_pk_add_f16 v170, v170, v58\n\t" \
    "v_pk_add_f16 v171, v171, v59\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v173, v168\n\t" \
    "v_cvt_f32_f16_sdwa v175, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v173, v173, v175\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_pk_add_f16 v164, v0, v1\n\t" \
    "v_pk_add_f16 v165, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "v_pk_add_f16 v166, v8, v9\n\t" \
    "v_pk_add_f16 v167, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:24576\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[96:99], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:26624\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:30720\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v164, v164, v16\n\t" \
    "v_pk_add_f16 v165, v165, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_pk_add_f16 v166, v166, v18\n\t" \
    "v_pk_add_f16 v167, v167, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[112:115], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v164, v164, v24\n\t" \
    "v_pk_add_f16 v165, v165, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_pk_add_f16 v166, v166, v26\n\t" \
    "v_pk_add_f16 v167, v167, v27\n\t" \
    "v_pk_add_f16 v164, v164, v165\n\t" \
    "v_pk_add_f16 v166, v166, v167\n\t" \
    "v_pk_add_f16 v164, v164, v166\n\t" \
    "v_cvt_f32_f16_e32 v172, v164\n\t" \
    "v_cvt_f32_f16_sdwa v174, v164 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v172, v172, v174\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[96:99], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:4096\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:4096\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:4096\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:4096\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "v_pk_add_f16 v168, v32, v33\n\t" \
    "v_pk_add_f16 v169, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[112:115], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "v_pk_add_f16 v170, v40, v41\n\t" \
    "v_pk_add_f16 v171, v42, v43\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v168, v168, v48\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "v_pk_add_f16 v169, v169, v49\n\t" \
    "v_pk_add_f16 v170, v170, v50\n\t" \
    "v_pk_add_f16 v171, v171, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[112:115], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v168, v168, v56\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_pk_add_f16 v169, v169, v57\n\t" \
    "v_pk_add_f16 v170, v170, v58\n\t" \
    "v_pk_add_f16 v171, v171, v59\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v173, v168\n\t" \
    "v_cvt_f32_f16_sdwa v175, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v173, v173, v175\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_pk_add_f16 v164, v0, v1\n\t" \
    "v_pk_add_f16 v165, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "v_pk_add_f16 v166, v8, v9\n\t" \
    "v_pk_add_f16 v167, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:16384\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[96:99], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:18432\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:22528\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v164, v164, v16\n\t" \
    "v_pk_add_f16 v165, v165, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_pk_add_f16 v166, v166, v18\n\t" \
    "v_pk_add_f16 v167, v167, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[112:115], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v164, v164, v24\n\t" \
    "v_pk_add_f16 v165, v165, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_pk_add_f16 v166, v166, v26\n\t" \
    "v_pk_add_f16 v167, v167, v27\n\t" \
    "v_pk_add_f16 v164, v164, v165\n\t" \
    "v_pk_add_f16 v166, v166, v167\n\t" \
    "v_pk_add_f16 v164, v164, v166\n\t" \
    "v_cvt_f32_f16_e32 v172, v164\n\t" \
    "v_cvt_f32_f16_sdwa v174, v164 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v172, v172, v174\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:8192\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:8192\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[96:99], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:8192\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:8192\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:12288\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:12288\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:12288\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:12288\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "v_pk_add_f16 v168, v32, v33\n\t" \
    "v_pk_add_f16 v169, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[112:115], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "v_pk_add_f16 v170, v40, v41\n\t" \
    "v_pk_add_f16 v171, v42, v43\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v168, v168, v48\n\t" \
    "v_pk_add_f16 v169, v169, v49\n\t" \
    "v_pk_add_f16 v170, v170, v50\n\t" \
    "v_pk_add_f16 v171, v171, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v168, v168, v56\n\t" \
    "v_pk_add_f16 v169, v169, v57\n\t" \
    "v_pk_add_f16 v170, v170, v58\n\t" \
    "v_pk_add_f16 v171, v171, v59\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v173, v168\n\t" \
    "v_cvt_f32_f16_sdwa v175, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v173, v173, v175\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:8704\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:8736\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:8768\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:8800\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:8832\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:8864\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:8896\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:8928\n\t" \
    "v_mov_b32 %[om0], v160\n\t" \
    "v_mov_b32 %[ol0], v162\n\t" \
    "v_mov_b32 %[om1], v161\n\t" \
    "v_mov_b32 %[ol1], v163\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS_ASM_D64_BF16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v162, 0\n\t" \
    "v_mov_b32 v163, 0\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "ds_read_b128 a[64:67], v0 offset:0\n\t" \
    "ds_read_b128 a[68:71], v1 offset:0\n\t" \
    "ds_read_b128 a[72:75], v2 offset:0\n\t" \
    "ds_read_b128 a[76:79], v3 offset:0\n\t" \
    "ds_read_b128 a[80:83], v0 offset:4096\n\t" \
    "ds_read_b128 a[84:87], v1 offset:4096\n\t" \
    "ds_read_b128 a[88:91], v2 offset:4096\n\t" \
    "ds_read_b128 a[92:95], v3 offset:4096\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:4096\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:4096\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:4096\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[64:67], 0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[112:115], a[64:67], 0\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[96:99], a[80:83], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[112:115], a[80:83], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_max3_f32 v160, v0, v1, v2\n\t" \
    "v_max3_f32 v160, v160, v3, v4\n\t" \
    "v_max3_f32 v160, v160, v5, v6\n\t" \
    "v_max3_f32 v160, v160, v7, v8\n\t" \
    "v_max3_f32 v160, v160, v9, v10\n\t" \
    "v_max3_f32 v160, v160, v11, v12\n\t" \
    "v_max3_f32 v160, v160, v13, v14\n\t" \
    "v_max3_f32 v160, v160, v15, v16\n\t" \
    "v_max3_f32 v160, v160, v17, v18\n\t" \
    "v_max3_f32 v160, v160, v19, v20\n\t" \
    "v_max3_f32 v160, v160, v21, v22\n\t" \
    "v_max3_f32 v160, v160, v23, v24\n\t" \
    "v_max3_f32 v160, v160, v25, v26\n\t" \
    "v_max3_f32 v160, v160, v27, v28\n\t" \
    "v_max3_f32 v160, v160, v29, v30\n\t" \
    "v_max_f32 v160, v160, v31\n\t" \
    "v_mov_b32 v174, v160\n\t" \
    "v_mov_b32 v175, v160\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v174, v175\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v160, v174, v175\n\t" \
    "v_max3_f32 v161, v32, v33, v34\n\t" \
    "v_max3_f32 v161, v161, v35, v36\n\t" \
    "v_max3_f32 v161, v161, v37, v38\n\t" \
    "v_max3_f32 v161, v161, v39, v40\n\t" \
    "v_max3_f32 v161, v161, v41, v42\n\t" \
    "v_max3_f32 v161, v161, v43, v44\n\t" \
    "v_max3_f32 v161, v161, v45, v46\n\t" \
    "v_max3_f32 v161, v161, v47, v48\n\t" \
    "v_max3_f32 v161, v161, v49, v50\n\t" \
    "v_max3_f32 v161, v161, v51, v52\n\t" \
    "v_max3_f32 v161, v161, v53, v54\n\t" \
    "v_max3_f32 v161, v161, v55, v56\n\t" \
    "v_max3_f32 v161, v161, v57, v58\n\t" \
    "v_max3_f32 v161, v161, v59, v60\n\t" \
    "v_max3_f32 v161, v161, v61, v62\n\t" \
    "v_max_f32 v161, v161, v63\n\t" \
    "v_mov_b32 v174, v161\n\t" \
    "v_mov_b32 v175, v161\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v174, v175\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v161, v174, v175\n\t" \
    "v_sub_f32 v64, 0, v160\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v160\n\t" \
    "v_sub_f32 v1, v1, v160\n\t" \
    "v_sub_f32 v2, v2, v160\n\t" \
    "v_sub_f32 v3, v3, v160\n\t" \
    "v_sub_f32 v4, v4, v160\n\t" \
    "v_sub_f32 v5, v5, v160\n\t" \
    "v_sub_f32 v6, v6, v160\n\t" \
    "v_sub_f32 v7, v7, v160\n\t" \
    "v_sub_f32 v8, v8, v160\n\t" \
    "v_sub_f32 v9, v9, v160\n\t" \
    "v_sub_f32 v10, v10, v160\n\t" \
    "v_sub_f32 v11, v11, v160\n\t" \
    "v_sub_f32 v12, v12, v160\n\t" \
    "v_sub_f32 v13, v13, v160\n\t" \
    "v_sub_f32 v14, v14, v160\n\t" \
    "v_sub_f32 v15, v15, v160\n\t" \
    "v_sub_f32 v16, v16, v160\n\t" \
    "v_sub_f32 v17, v17, v160\n\t" \
    "v_sub_f32 v18, v18, v160\n\t" \
    "v_sub_f32 v19, v19, v160\n\t" \
    "v_sub_f32 v20, v20, v160\n\t" \
    "v_sub_f32 v21, v21, v160\n\t" \
    "v_sub_f32 v22, v22, v160\n\t" \
    "v_sub_f32 v23, v23, v160\n\t" \
    "v_sub_f32 v24, v24, v160\n\t" \
    "v_sub_f32 v25, v25, v160\n\t" \
    "v_sub_f32 v26, v26, v160\n\t" \
    "v_sub_f32 v27, v27, v160\n\t" \
    "v_sub_f32 v28, v28, v160\n\t" \
    "v_sub_f32 v29, v29, v160\n\t" \
    "v_sub_f32 v30, v30, v160\n\t" \
    "v_sub_f32 v31, v31, v160\n\t" \
    "v_sub_f32 v80, 0, v161\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v161\n\t" \
    "v_sub_f32 v33, v33, v161\n\t" \
    "v_sub_f32 v34, v34, v161\n\t" \
    "v_sub_f32 v35, v35, v161\n\t" \
    "v_sub_f32 v36, v36, v161\n\t" \
    "v_sub_f32 v37, v37, v161\n\t" \
    "v_sub_f32 v38, v38, v161\n\t" \
    "v_sub_f32 v39, v39, v161\n\t" \
    "v_sub_f32 v40, v40, v161\n\t" \
    "v_sub_f32 v41, v41, v161\n\t" \
    "v_sub_f32 v42, v42, v161\n\t" \
    "v_sub_f32 v43, v43, v161\n\t" \
    "v_sub_f32 v44, v44, v161\n\t" \
    "v_sub_f32 v45, v45, v161\n\t" \
    "v_sub_f32 v46, v46, v161\n\t" \
    "v_sub_f32 v47, v47, v161\n\t" \
    "v_sub_f32 v48, v48, v161\n\t" \
    "v_sub_f32 v49, v49, v161\n\t" \
    "v_sub_f32 v50, v50, v161\n\t" \
    "v_sub_f32 v51, v51, v161\n\t" \
    "v_sub_f32 v52, v52, v161\n\t" \
    "v_sub_f32 v53, v53, v161\n\t" \
    "v_sub_f32 v54, v54, v161\n\t" \
    "v_sub_f32 v55, v55, v161\n\t" \
    "v_sub_f32 v56, v56, v161\n\t" \
    "v_sub_f32 v57, v57, v161\n\t" \
    "v_sub_f32 v58, v58, v161\n\t" \
    "v_sub_f32 v59, v59, v161\n\t" \
    "v_sub_f32 v60, v60, v161\n\t" \
    "v_sub_f32 v61, v61, v161\n\t" \
    "v_sub_f32 v62, v62, v161\n\t" \
    "v_sub_f32 v63, v63, v161\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v164, v0, v4\n\t" \
    "v_add_f32 v165, v1, v5\n\t" \
    "v_add_f32 v166, v2, v6\n\t" \
    "v_add_f32 v167, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v164, v164, v8\n\t" \
    "v_add_f32 v164, v164, v12\n\t" \
    "v_add_f32 v165, v165, v9\n\t" \
    "v_add_f32 v165, v165, v13\n\t" \
    "v_add_f32 v166, v166, v10\n\t" \
    "v_add_f32 v166, v166, v14\n\t" \
    "v_add_f32 v167, v167, v11\n\t" \
    "v_add_f32 v167, v167, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v164, v164, v16\n\t" \
    "v_add_f32 v164, v164, v20\n\t" \
    "v_add_f32 v165, v165, v17\n\t" \
    "v_add_f32 v165, v165, v21\n\t" \
    "v_add_f32 v166, v166, v18\n\t" \
    "v_add_f32 v166, v166, v22\n\t" \
    "v_add_f32 v167, v167, v19\n\t" \
    "v_add_f32 v167, v167, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v164, v164, v24\n\t" \
    "v_add_f32 v164, v164, v28\n\t" \
    "v_add_f32 v165, v165, v25\n\t" \
    "v_add_f32 v165, v165, v29\n\t" \
    "v_add_f32 v166, v166, v26\n\t" \
    "v_add_f32 v166, v166, v30\n\t" \
    "v_add_f32 v167, v167, v27\n\t" \
    "v_add_f32 v167, v167, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v164, v164, v165\n\t" \
    "v_add_f32 v166, v166, v167\n\t" \
    "v_add_f32 v172, v164, v166\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v168, v32, v36\n\t" \
    "v_add_f32 v169, v33, v37\n\t" \
    "v_add_f32 v170, v34, v38\n\t" \
    "v_add_f32 v171, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v168, v168, v40\n\t" \
    "v_add_f32 v168, v168, v44\n\t" \
    "v_add_f32 v169, v169, v41\n\t" \
    "v_add_f32 v169, v169, v45\n\t" \
    "v_add_f32 v170, v170, v42\n\t" \
    "v_add_f32 v170, v170, v46\n\t" \
    "v_add_f32 v171, v171, v43\n\t" \
    "v_add_f32 v171, v171, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:22528\n\t" \
    "v_accvgpr_write_b32 a32, 0\n\t" \
    "v_accvgpr_write_b32 a33, 0\n\t" \
    "v_accvgpr_write_b32 a34, 0\n\t" \
    "v_accvgpr_write_b32 a35, 0\n\t" \
    "v_accvgpr_write_b32 a36, 0\n\t" \
    "v_accvgpr_write_b32 a37, 0\n\t" \
    "v_accvgpr_write_b32 a38, 0\n\t" \
    "v_accvgpr_write_b32 a39, 0\n\t" \
    "v_accvgpr_write_b32 a40, 0\n\t" \
    "v_accvgpr_write_b32 a41, 0\n\t" \
    "v_accvgpr_write_b32 a42, 0\n\t" \
    "v_accvgpr_write_b32 a43, 0\n\t" \
    "v_accvgpr_write_b32 a44, 0\n\t" \
    "v_accvgpr_write_b32 a45, 0\n\t" \
    "v_accvgpr_write_b32 a46, 0\n\t" \
    "v_accvgpr_write_b32 a47, 0\n\t" \
    "v_accvgpr_write_b32 a48, 0\n\t" \
    "v_accvgpr_write_b32 a49, 0\n\t" \
    "v_accvgpr_write_b32 a50, 0\n\t" \
    "v_accvgpr_write_b32 a51, 0\n\t" \
    "v_accvgpr_write_b32 a52, 0\n\t" \
    "v_accvgpr_write_b32 a53, 0\n\t" \
    "v_accvgpr_write_b32 a54, 0\n\t" \
    "v_accvgpr_write_b32 a55, 0\n\t" \
    "v_accvgpr_write_b32 a56, 0\n\t" \
    "v_accvgpr_write_b32 a57, 0\n\t" \
    "v_accvgpr_write_b32 a58, 0\n\t" \
    "v_accvgpr_write_b32 a59, 0\n\t" \
    "v_accvgpr_write_b32 a60, 0\n\t" \
    "v_accvgpr_write_b32 a61, 0\n\t" \
    "v_accvgpr_write_b32 a62, 0\n\t" \
    "v_accvgpr_write_b32 a63, 0\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[96:99], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[112:115], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:8192\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:8192\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:8192\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:8192\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:12288\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:12288\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:12288\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:12288\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v168, v168, v48\n\t" \
    "v_add_f32 v168, v168, v52\n\t" \
    "v_add_f32 v169, v169, v49\n\t" \
    "v_add_f32 v169, v169, v53\n\t" \
    "v_add_f32 v170, v170, v50\n\t" \
    "v_add_f32 v170, v170, v54\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "v_add_f32 v171, v171, v51\n\t" \
    "v_add_f32 v171, v171, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[112:115], a[64:67], v[64:79]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v168, v168, v56\n\t" \
    "v_add_f32 v168, v168, v60\n\t" \
    "v_add_f32 v169, v169, v57\n\t" \
    "v_add_f32 v169, v169, v61\n\t" \
    "v_add_f32 v170, v170, v58\n\t" \
    "v_add_f32 v170, v170, v62\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_add_f32 v171, v171, v59\n\t" \
    "v_add_f32 v171, v171, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v173, v168, v170\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v164, v0, v4\n\t" \
    "v_add_f32 v165, v1, v5\n\t" \
    "v_add_f32 v166, v2, v6\n\t" \
    "v_add_f32 v167, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v164, v164, v8\n\t" \
    "v_add_f32 v164, v164, v12\n\t" \
    "v_add_f32 v165, v165, v9\n\t" \
    "v_add_f32 v165, v165, v13\n\t" \
    "v_add_f32 v166, v166, v10\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "v_add_f32 v166, v166, v14\n\t" \
    "v_add_f32 v167, v167, v11\n\t" \
    "v_add_f32 v167, v167, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:24576\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[96:99], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:26624\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:30720\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v164, v164, v16\n\t" \
    "v_add_f32 v164, v164, v20\n\t" \
    "v_add_f32 v165, v165, v17\n\t" \
    "v_add_f32 v165, v165, v21\n\t" \
    "v_add_f32 v166, v166, v18\n\t" \
    "v_add_f32 v166, v166, v22\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_add_f32 v167, v167, v19\n\t" \
    "v_add_f32 v167, v167, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[112:115], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v164, v164, v24\n\t" \
    "v_add_f32 v164, v164, v28\n\t" \
    "v_add_f32 v165, v165, v25\n\t" \
    "v_add_f32 v165, v165, v29\n\t" \
    "v_add_f32 v166, v166, v26\n\t" \
    "v_add_f32 v166, v166, v30\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_add_f32 v167, v167, v27\n\t" \
    "v_add_f32 v167, v167, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v164, v164, v165\n\t" \
    "v_add_f32 v166, v166, v167\n\t" \
    "v_add_f32 v172, v164, v166\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[96:99], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:4096\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:4096\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:4096\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:4096\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v168, v32, v36\n\t" \
    "v_add_f32 v169, v33, v37\n\t" \
    "v_add_f32 v170, v34, v38\n\t" \
    "v_add_f32 v171, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[112:115], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v168, v168, v40\n\t" \
    "v_add_f32 v168, v168, v44\n\t" \
    "v_add_f32 v169, v169, v41\n\t" \
    "v_add_f32 v169, v169, v45\n\t" \
    "v_add_f32 v170, v170, v42\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "v_add_f32 v170, v170, v46\n\t" \
    "v_add_f32 v171, v171, v43\n\t" \
    "v_add_f32 v171, v171, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[64:67], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[68:71], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[72:75], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v168, v168, v48\n\t" \
    "v_add_f32 v168, v168, v52\n\t" \
    "v_add_f32 v169, v169, v49\n\t" \
    "v_add_f32 v169, v169, v53\n\t" \
    "v_add_f32 v170, v170, v50\n\t" \
    "v_add_f32 v170, v170, v54\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[76:79], v[0:15]\n\t" \
    "v_add_f32 v171, v171, v51\n\t" \
    "v_add_f32 v171, v171, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[112:115], a[64:67], v[64:79]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[116:119], a[68:71], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[120:123], a[72:75], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v168, v168, v56\n\t" \
    "v_add_f32 v168, v168, v60\n\t" \
    "v_add_f32 v169, v169, v57\n\t" \
    "v_add_f32 v169, v169, v61\n\t" \
    "v_add_f32 v170, v170, v58\n\t" \
    "v_add_f32 v170, v170, v62\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[124:127], a[76:79], v[16:31]\n\t" \
    "v_add_f32 v171, v171, v59\n\t" \
    "v_add_f32 v171, v171, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v173, v168, v170\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v164, v0, v4\n\t" \
    "v_add_f32 v165, v1, v5\n\t" \
    "v_add_f32 v166, v2, v6\n\t" \
    "v_add_f32 v167, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v164, v164, v8\n\t" \
    "v_add_f32 v164, v164, v12\n\t" \
    "v_add_f32 v165, v165, v9\n\t" \
    "v_add_f32 v165, v165, v13\n\t" \
    "v_add_f32 v166, v166, v10\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "v_add_f32 v166, v166, v14\n\t" \
    "v_add_f32 v167, v167, v11\n\t" \
    "v_add_f32 v167, v167, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[96:97], %[va0_0] offset:16384\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[98:99], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[100:101], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[102:103], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[104:105], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[106:107], %[va0_1] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[96:99], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[108:109], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[110:111], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[112:113], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[114:115], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[116:117], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[118:119], %[va1_1] offset:18432\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[100:103], a[84:87], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[120:121], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[122:123], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[124:125], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[126:127], %[va1_1] offset:22528\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[104:107], a[88:91], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v164, v164, v16\n\t" \
    "v_add_f32 v164, v164, v20\n\t" \
    "v_add_f32 v165, v165, v17\n\t" \
    "v_add_f32 v165, v165, v21\n\t" \
    "v_add_f32 v166, v166, v18\n\t" \
    "v_add_f32 v166, v166, v22\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[108:111], a[92:95], v[32:47]\n\t" \
    "v_add_f32 v167, v167, v19\n\t" \
    "v_add_f32 v167, v167, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[112:115], a[80:83], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[116:119], a[84:87], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[120:123], a[88:91], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v164, v164, v24\n\t" \
    "v_add_f32 v164, v164, v28\n\t" \
    "v_add_f32 v165, v165, v25\n\t" \
    "v_add_f32 v165, v165, v29\n\t" \
    "v_add_f32 v166, v166, v26\n\t" \
    "v_add_f32 v166, v166, v30\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[124:127], a[92:95], v[48:63]\n\t" \
    "v_add_f32 v167, v167, v27\n\t" \
    "v_add_f32 v167, v167, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v164, v164, v165\n\t" \
    "v_add_f32 v166, v166, v167\n\t" \
    "v_add_f32 v172, v164, v166\n\t" \
    "v_add_f32 v162, v162, v172\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v172\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:8192\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:8192\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:8192\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[96:99], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:8192\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:12288\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:12288\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[100:103], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:12288\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:12288\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[104:107], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v168, v32, v36\n\t" \
    "v_add_f32 v169, v33, v37\n\t" \
    "v_add_f32 v170, v34, v38\n\t" \
    "v_add_f32 v171, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[108:111], v[24:27], a[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[112:115], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[116:119], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[120:123], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v168, v168, v40\n\t" \
    "v_add_f32 v168, v168, v44\n\t" \
    "v_add_f32 v169, v169, v41\n\t" \
    "v_add_f32 v169, v169, v45\n\t" \
    "v_add_f32 v170, v170, v42\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[124:127], v[24:27], a[16:31]\n\t" \
    "v_add_f32 v170, v170, v46\n\t" \
    "v_add_f32 v171, v171, v43\n\t" \
    "v_add_f32 v171, v171, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v168, v168, v48\n\t" \
    "v_add_f32 v168, v168, v52\n\t" \
    "v_add_f32 v169, v169, v49\n\t" \
    "v_add_f32 v169, v169, v53\n\t" \
    "v_add_f32 v170, v170, v50\n\t" \
    "v_add_f32 v170, v170, v54\n\t" \
    "v_add_f32 v171, v171, v51\n\t" \
    "v_add_f32 v171, v171, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v168, v168, v56\n\t" \
    "v_add_f32 v168, v168, v60\n\t" \
    "v_add_f32 v169, v169, v57\n\t" \
    "v_add_f32 v169, v169, v61\n\t" \
    "v_add_f32 v170, v170, v58\n\t" \
    "v_add_f32 v170, v170, v62\n\t" \
    "v_add_f32 v171, v171, v59\n\t" \
    "v_add_f32 v171, v171, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v173, v168, v170\n\t" \
    "v_add_f32 v163, v163, v173\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v173\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[96:99], v[32:35], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[100:103], v[40:43], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[104:107], v[48:51], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[108:111], v[56:59], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[112:115], v[32:35], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[116:119], v[40:43], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[120:123], v[48:51], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[124:127], v[56:59], a[48:63]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:8704\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:8736\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:8768\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:8800\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:8832\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:8864\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:8896\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:8928\n\t" \
    "v_mov_b32 %[om0], v160\n\t" \
    "v_mov_b32 %[ol0], v162\n\t" \
    "v_mov_b32 %[om1], v161\n\t" \
    "v_mov_b32 %[ol1], v163\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS_OUTPUTS_D64 [om0] "=&v"(hs_m0), [om1] "=&v"(hs_m1), [ol0] "=&v"(hs_l0), [ol1] "=&v"(hs_l1), [flg] "=&s"(hs_flag), [cnt] "+s"(hs_cnt), [goff] "+s"(hs_goff)
#define FA2_HS_INPUTS_D64 [ka0] "v"(hs_ka[0]), [ka1] "v"(hs_ka[1]), [ka2] "v"(hs_ka[2]), [ka3] "v"(hs_ka[3]), [va0_0] "v"(hs_va[0][0]), [va0_1] "v"(hs_va[0][1]), [va1_0] "v"(hs_va[1][0]), [va1_1] "v"(hs_va[1][1]), [vo0] "v"(hs_vo[0]), [vo1] "v"(hs_vo[1]), [lo] "v"(hs_lo), [oa] "v"(hs_oa), [rsk] "s"(hs_rsk), [rsv] "s"(hs_rsv), [qb] "s"(hs_qb)
#define FA2_HS_CLOBBERS_D64 "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "vcc", "scc", "memory"
#define FA2_HS_LDS_D64 69632

#define FA2_HS_ASM_D128_F16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v210, 0\n\t" \
    "v_mov_b32 v211, 0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "v_add_u32 v4, %[qb], %[ka4]\n\t" \
    "v_add_u32 v5, %[qb], %[ka5]\n\t" \
    "v_add_u32 v6, %[qb], %[ka6]\n\t" \
    "v_add_u32 v7, %[qb], %[ka7]\n\t" \
    "ds_read_b128 a[128:131], v0 offset:0\n\t" \
    "ds_read_b128 a[132:135], v1 offset:0\n\t" \
    "ds_read_b128 a[136:139], v2 offset:0\n\t" \
    "ds_read_b128 a[140:143], v3 offset:0\n\t" \
    "ds_read_b128 a[144:147], v4 offset:0\n\t" \
    "ds_read_b128 a[148:151], v5 offset:0\n\t" \
    "ds_read_b128 a[152:155], v6 offset:0\n\t" \
    "ds_read_b128 a[156:159], v7 offset:0\n\t" \
    "ds_read_b128 a[160:163], v0 offset:8192\n\t" \
    "ds_read_b128 a[164:167], v1 offset:8192\n\t" \
    "ds_read_b128 a[168:171], v2 offset:8192\n\t" \
    "ds_read_b128 a[172:175], v3 offset:8192\n\t" \
    "ds_read_b128 a[176:179], v4 offset:8192\n\t" \
    "ds_read_b128 a[180:183], v5 offset:8192\n\t" \
    "ds_read_b128 a[184:187], v6 offset:8192\n\t" \
    "ds_read_b128 a[188:191], v7 offset:8192\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:0\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:0\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:0\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:0\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:8192\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:8192\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:8192\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:8192\n\t" \
    "ds_read_b128 v[64:67], %[ka4] offset:8192\n\t" \
    "ds_read_b128 v[68:71], %[ka5] offset:8192\n\t" \
    "ds_read_b128 v[72:75], %[ka6] offset:8192\n\t" \
    "ds_read_b128 v[76:79], %[ka7] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[128:131], 0\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(13)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[128:131], a[128:131], 0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[64:67], a[144:147], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[68:71], a[148:151], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[72:75], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[76:79], a[156:159], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[96:99], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[100:103], a[164:167], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[104:107], a[168:171], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[108:111], a[172:175], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[112:115], a[176:179], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[128:131], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[64:67], a[176:179], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[68:71], a[180:183], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[72:75], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[76:79], a[188:191], v[48:63]\n\t" \
    "v_max3_f32 v208, v0, v1, v2\n\t" \
    "v_max3_f32 v208, v208, v3, v4\n\t" \
    "v_max3_f32 v208, v208, v5, v6\n\t" \
    "v_max3_f32 v208, v208, v7, v8\n\t" \
    "v_max3_f32 v208, v208, v9, v10\n\t" \
    "v_max3_f32 v208, v208, v11, v12\n\t" \
    "v_max3_f32 v208, v208, v13, v14\n\t" \
    "v_max3_f32 v208, v208, v15, v16\n\t" \
    "v_max3_f32 v208, v208, v17, v18\n\t" \
    "v_max3_f32 v208, v208, v19, v20\n\t" \
    "v_max3_f32 v208, v208, v21, v22\n\t" \
    "v_max3_f32 v208, v208, v23, v24\n\t" \
    "v_max3_f32 v208, v208, v25, v26\n\t" \
    "v_max3_f32 v208, v208, v27, v28\n\t" \
    "v_max3_f32 v208, v208, v29, v30\n\t" \
    "v_max_f32 v208, v208, v31\n\t" \
    "v_mov_b32 v222, v208\n\t" \
    "v_mov_b32 v223, v208\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v222, v223\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v208, v222, v223\n\t" \
    "v_max3_f32 v209, v32, v33, v34\n\t" \
    "v_max3_f32 v209, v209, v35, v36\n\t" \
    "v_max3_f32 v209, v209, v37, v38\n\t" \
    "v_max3_f32 v209, v209, v39, v40\n\t" \
    "v_max3_f32 v209, v209, v41, v42\n\t" \
    "v_max3_f32 v209, v209, v43, v44\n\t" \
    "v_max3_f32 v209, v209, v45, v46\n\t" \
    "v_max3_f32 v209, v209, v47, v48\n\t" \
    "v_max3_f32 v209, v209, v49, v50\n\t" \
    "v_max3_f32 v209, v209, v51, v52\n\t" \
    "v_max3_f32 v209, v209, v53, v54\n\t" \
    "v_max3_f32 v209, v209, v55, v56\n\t" \
    "v_max3_f32 v209, v209, v57, v58\n\t" \
    "v_max3_f32 v209, v209, v59, v60\n\t" \
    "v_max3_f32 v209, v209, v61, v62\n\t" \
    "v_max_f32 v209, v209, v63\n\t" \
    "v_mov_b32 v222, v209\n\t" \
    "v_mov_b32 v223, v209\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v222, v223\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v209, v222, v223\n\t" \
    "v_sub_f32 v64, 0, v208\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v208\n\t" \
    "v_sub_f32 v1, v1, v208\n\t" \
    "v_sub_f32 v2, v2, v208\n\t" \
    "v_sub_f32 v3, v3, v208\n\t" \
    "v_sub_f32 v4, v4, v208\n\t" \
    "v_sub_f32 v5, v5, v208\n\t" \
    "v_sub_f32 v6, v6, v208\n\t" \
    "v_sub_f32 v7, v7, v208\n\t" \
    "v_sub_f32 v8, v8, v208\n\t" \
    "v_sub_f32 v9, v9, v208\n\t" \
    "v_sub_f32 v10, v10, v208\n\t" \
    "v_sub_f32 v11, v11, v208\n\t" \
    "v_sub_f32 v12, v12, v208\n\t" \
    "v_sub_f32 v13, v13, v208\n\t" \
    "v_sub_f32 v14, v14, v208\n\t" \
    "v_sub_f32 v15, v15, v208\n\t" \
    "v_sub_f32 v16, v16, v208\n\t" \
    "v_sub_f32 v17, v17, v208\n\t" \
    "v_sub_f32 v18, v18, v208\n\t" \
    "v_sub_f32 v19, v19, v208\n\t" \
    "v_sub_f32 v20, v20, v208\n\t" \
    "v_sub_f32 v21, v21, v208\n\t" \
    "v_sub_f32 v22, v22, v208\n\t" \
    "v_sub_f32 v23, v23, v208\n\t" \
    "v_sub_f32 v24, v24, v208\n\t" \
    "v_sub_f32 v25, v25, v208\n\t" \
    "v_sub_f32 v26, v26, v208\n\t" \
    "v_sub_f32 v27, v27, v208\n\t" \
    "v_sub_f32 v28, v28, v208\n\t" \
    "v_sub_f32 v29, v29, v208\n\t" \
    "v_sub_f32 v30, v30, v208\n\t" \
    "v_sub_f32 v31, v31, v208\n\t" \
    "v_sub_f32 v80, 0, v209\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v209\n\t" \
    "v_sub_f32 v33, v33, v209\n\t" \
    "v_sub_f32 v34, v34, v209\n\t" \
    "v_sub_f32 v35, v35, v209\n\t" \
    "v_sub_f32 v36, v36, v209\n\t" \
    "v_sub_f32 v37, v37, v209\n\t" \
    "v_sub_f32 v38, v38, v209\n\t" \
    "v_sub_f32 v39, v39, v209\n\t" \
    "v_sub_f32 v40, v40, v209\n\t" \
    "v_sub_f32 v41, v41, v209\n\t" \
    "v_sub_f32 v42, v42, v209\n\t" \
    "v_sub_f32 v43, v43, v209\n\t" \
    "v_sub_f32 v44, v44, v209\n\t" \
    "v_sub_f32 v45, v45, v209\n\t" \
    "v_sub_f32 v46, v46, v209\n\t" \
    "v_sub_f32 v47, v47, v209\n\t" \
    "v_sub_f32 v48, v48, v209\n\t" \
    "v_sub_f32 v49, v49, v209\n\t" \
    "v_sub_f32 v50, v50, v209\n\t" \
    "v_sub_f32 v51, v51, v209\n\t" \
    "v_sub_f32 v52, v52, v209\n\t" \
    "v_sub_f32 v53, v53, v209\n\t" \
    "v_sub_f32 v54, v54, v209\n\t" \
    "v_sub_f32 v55, v55, v209\n\t" \
    "v_sub_f32 v56, v56, v209\n\t" \
    "v_sub_f32 v57, v57, v209\n\t" \
    "v_sub_f32 v58, v58, v209\n\t" \
    "v_sub_f32 v59, v59, v209\n\t" \
    "v_sub_f32 v60, v60, v209\n\t" \
    "v_sub_f32 v61, v61, v209\n\t" \
    "v_sub_f32 v62, v62, v209\n\t" \
    "v_sub_f32 v63, v63, v209\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v212, v0, v1\n\t" \
    "v_pk_add_f16 v213, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v214, v8, v9\n\t" \
    "v_pk_add_f16 v215, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v212, v212, v16\n\t" \
    "v_pk_add_f16 v213, v213, v17\n\t" \
    "v_pk_add_f16 v214, v214, v18\n\t" \
    "v_pk_add_f16 v215, v215, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v212, v212, v24\n\t" \
    "v_pk_add_f16 v213, v213, v25\n\t" \
    "v_pk_add_f16 v214, v214, v26\n\t" \
    "v_pk_add_f16 v215, v215, v27\n\t" \
    "v_pk_add_f16 v212, v212, v213\n\t" \
    "v_pk_add_f16 v214, v214, v215\n\t" \
    "v_pk_add_f16 v212, v212, v214\n\t" \
    "v_cvt_f32_f16_e32 v220, v212\n\t" \
    "v_cvt_f32_f16_sdwa v222, v212 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v220, v220, v222\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v216, v32, v33\n\t" \
    "v_pk_add_f16 v217, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v218, v40, v41\n\t" \
    "v_pk_add_f16 v219, v42, v43\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:45056\n\t" \
    "v_accvgpr_write_b32 a64, 0\n\t" \
    "v_accvgpr_write_b32 a65, 0\n\t" \
    "v_accvgpr_write_b32 a66, 0\n\t" \
    "v_accvgpr_write_b32 a67, 0\n\t" \
    "v_accvgpr_write_b32 a68, 0\n\t" \
    "v_accvgpr_write_b32 a69, 0\n\t" \
    "v_accvgpr_write_b32 a70, 0\n\t" \
    "v_accvgpr_write_b32 a71, 0\n\t" \
    "v_accvgpr_write_b32 a72, 0\n\t" \
    "v_accvgpr_write_b32 a73, 0\n\t" \
    "v_accvgpr_write_b32 a74, 0\n\t" \
    "v_accvgpr_write_b32 a75, 0\n\t" \
    "v_accvgpr_write_b32 a76, 0\n\t" \
    "v_accvgpr_write_b32 a77, 0\n\t" \
    "v_accvgpr_write_b32 a78, 0\n\t" \
    "v_accvgpr_write_b32 a79, 0\n\t" \
    "v_accvgpr_write_b32 a80, 0\n\t" \
    "v_accvgpr_write_b32 a81, 0\n\t" \
    "v_accvgpr_write_b32 a82, 0\n\t" \
    "v_accvgpr_write_b32 a83, 0\n\t" \
    "v_accvgpr_write_b32 a84, 0\n\t" \
    "v_accvgpr_write_b32 a85, 0\n\t" \
    "v_accvgpr_write_b32 a86, 0\n\t" \
    "v_accvgpr_write_b32 a87, 0\n\t" \
    "v_accvgpr_write_b32 a88, 0\n\t" \
    "v_accvgpr_write_b32 a89, 0\n\t" \
    "v_accvgpr_write_b32 a90, 0\n\t" \
    "v_accvgpr_write_b32 a91, 0\n\t" \
    "v_accvgpr_write_b32 a92, 0\n\t" \
    "v_accvgpr_write_b32 a93, 0\n\t" \
    "v_accvgpr_write_b32 a94, 0\n\t" \
    "v_accvgpr_write_b32 a95, 0\n\t" \
    "v_accvgpr_write_b32 a96, 0\n\t" \
    "v_accvgpr_write_b32 a97, 0\n\t" \
    "v_accvgpr_write_b32 a98, 0\n\t" \
    "v_accvgpr_write_b32 a99, 0\n\t" \
    "v_accvgpr_write_b32 a100, 0\n\t" \
    "v_accvgpr_write_b32 a101, 0\n\t" \
    "v_accvgpr_write_b32 a102, 0\n\t" \
    "v_accvgpr_write_b32 a103, 0\n\t" \
    "v_accvgpr_write_b32 a104, 0\n\t" \
    "v_accvgpr_write_b32 a105, 0\n\t" \
    "v_accvgpr_write_b32 a106, 0\n\t" \
    "v_accvgpr_write_b32 a107, 0\n\t" \
    "v_accvgpr_write_b32 a108, 0\n\t" \
    "v_accvgpr_write_b32 a109, 0\n\t" \
    "v_accvgpr_write_b32 a110, 0\n\t" \
    "v_accvgpr_write_b32 a111, 0\n\t" \
    "v_accvgpr_write_b32 a112, 0\n\t" \
    "v_accvgpr_write_b32 a113, 0\n\t" \
    "v_accvgpr_write_b32 a114, 0\n\t" \
    "v_accvgpr_write_b32 a115, 0\n\t" \
    "v_accvgpr_write_b32 a116, 0\n\t" \
    "v_accvgpr_write_b32 a117, 0\n\t" \
    "v_accvgpr_write_b32 a118, 0\n\t" \
    "v_accvgpr_write_b32 a119, 0\n\t" \
    "v_accvgpr_write_b32 a120, 0\n\t" \
    "v_accvgpr_write_b32 a121, 0\n\t" \
    "v_accvgpr_write_b32 a122, 0\n\t" \
    "v_accvgpr_write_b32 a123, 0\n\t" \
    "v_accvgpr_write_b32 a124, 0\n\t" \
    "v_accvgpr_write_b32 a125, 0\n\t" \
    "v_accvgpr_write_b32 a126, 0\n\t" \
    "v_accvgpr_write_b32 a127, 0\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[224:227], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[240:243], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_f16_f32 v160, v160, v161\n\t" \
    "v_cvt_pk_f16_f32 v161, v162, v163\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_f16_f32 v162, v164, v165\n\t" \
    "v_cvt_pk_f16_f32 v163, v166, v167\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:24576\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_f16_f32 v168, v168, v169\n\t" \
    "v_cvt_pk_f16_f32 v169, v170, v171\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_f16_f32 v170, v172, v173\n\t" \
    "v_cvt_pk_f16_f32 v171, v174, v175\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:28672\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v176, v176, v177\n\t" \
    "v_cvt_pk_f16_f32 v177, v178, v179\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v178, v180, v181\n\t" \
    "v_cvt_pk_f16_f32 v179, v182, v183\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:49152\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v184, v184, v185\n\t" \
    "v_cvt_pk_f16_f32 v185, v186, v187\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v186, v188, v189\n\t" \
    "v_cvt_pk_f16_f32 v187, v190, v191\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:53248\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v192, v192, v193\n\t" \
    "v_cvt_pk_f16_f32 v193, v194, v195\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_f16_f32 v194, v196, v197\n\t" \
    "v_cvt_pk_f16_f32 v195, v198, v199\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:57344\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_f16_f32 v200, v200, v201\n\t" \
    "v_cvt_pk_f16_f32 v201, v202, v203\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_f16_f32 v202, v204, v205\n\t" \
    "v_cvt_pk_f16_f32 v203, v206, v207\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:61440\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:16384\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:16384\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:16384\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:16384\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:16384\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:16384\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:16384\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:16384\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:24576\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:24576\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:24576\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:24576\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[128:131], v[64:79]\n\t" \
    "ds_read_b128 v[96:99], %[ka4] offset:24576\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "ds_read_b128 v[100:103], %[ka5] offset:24576\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v216, v216, v48\n\t" \
    "v_pk_add_f16 v217, v217, v49\n\t" \
    "v_pk_add_f16 v218, v218, v50\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:0\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "v_pk_add_f16 v219, v219, v51\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "ds_read_b128 v[104:107], %[ka6] offset:24576\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_f16_f32 v160, v160, v161\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_f16_f32 v161, v162, v163\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_f16_f32 v162, v164, v165\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_cvt_pk_f16_f32 v163, v166, v167\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[128:131], a[128:131], v[64:79]\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:8192\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "ds_read_b128 v[108:111], %[ka7] offset:24576\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_f16_f32 v168, v168, v169\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v216, v216, v56\n\t" \
    "v_cvt_pk_f16_f32 v169, v170, v171\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "v_pk_add_f16 v217, v217, v57\n\t" \
    "v_pk_add_f16 v218, v218, v58\n\t" \
    "v_pk_add_f16 v219, v219, v59\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_f16_f32 v170, v172, v173\n\t" \
    "v_pk_add_f16 v216, v216, v217\n\t" \
    "v_pk_add_f16 v218, v218, v219\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v171, v174, v175\n\t" \
    "v_pk_add_f16 v216, v216, v218\n\t" \
    "v_cvt_f32_f16_e32 v221, v216\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:12288\n\t" \
    "v_cvt_f32_f16_sdwa v223, v216 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[96:99], a[144:147], v[16:31]\n\t" \
    "v_add_f32 v221, v221, v223\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[100:103], a[148:151], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[104:107], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[108:111], a[156:159], v[16:31]\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v176, v176, v177\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v177, v178, v179\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v178, v180, v181\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_cvt_pk_f16_f32 v179, v182, v183\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:49152\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:49152\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:32768\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v184, v184, v185\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:53248\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "v_cvt_pk_f16_f32 v185, v186, v187\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v186, v188, v189\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v187, v190, v191\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:53248\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:36864\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v212, v0, v1\n\t" \
    "v_pk_add_f16 v213, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v192, v192, v193\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:57344\n\t" \
    "v_cvt_pk_f16_f32 v193, v194, v195\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v194, v196, v197\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_cvt_pk_f16_f32 v195, v198, v199\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:57344\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:40960\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v200, v200, v201\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:61440\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_cvt_pk_f16_f32 v201, v202, v203\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v202, v204, v205\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v203, v206, v207\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:61440\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:45056\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v214, v8, v9\n\t" \
    "v_pk_add_f16 v215, v10, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:49152\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[112:115], a[176:179], v[80:95]\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:49152\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:53248\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:53248\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:57344\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:57344\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:61440\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:61440\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[128:131], a[160:163], v[80:95]\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:49152\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v212, v212, v16\n\t" \
    "v_pk_add_f16 v213, v213, v17\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:49152\n\t" \
    "v_pk_add_f16 v214, v214, v18\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_pk_add_f16 v215, v215, v19\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:53248\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:53248\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:16384\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:57344\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:16384\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:57344\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[112:115], a[160:163], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:61440\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:61440\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[116:119], a[164:167], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:49152\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:49152\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[120:123], a[168:171], v[32:47]\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:53248\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v212, v212, v24\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:53248\n\t" \
    "v_pk_add_f16 v213, v213, v25\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[124:127], a[172:175], v[32:47]\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_pk_add_f16 v214, v214, v26\n\t" \
    "v_pk_add_f16 v215, v215, v27\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:57344\n\t" \
    "v_pk_add_f16 v212, v212, v213\n\t" \
    "v_pk_add_f16 v214, v214, v215\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[96:99], a[176:179], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:57344\n\t" \
    "v_pk_add_f16 v212, v212, v214\n\t" \
    "v_cvt_f32_f16_e32 v220, v212\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:61440\n\t" \
    "v_cvt_f32_f16_sdwa v222, v212 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v220, v220, v222\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[100:103], a[180:183], v[48:63]\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:61440\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[104:107], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[108:111], a[188:191], v[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:0\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:0\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v216, v32, v33\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_pk_add_f16 v217, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[224:227], v[0:3], a[32:47]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:8192\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:8192\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:8192\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[240:243], v[0:3], a[48:63]\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:8192\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "v_pk_add_f16 v218, v40, v41\n\t" \
    "v_pk_add_f16 v219, v42, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[96:99], a[128:131], v[64:79]\n\t" \
    "ds_read_b128 v[96:99], %[ka4] offset:8192\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "ds_read_b128 v[100:103], %[ka5] offset:8192\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v216, v216, v48\n\t" \
    "v_pk_add_f16 v217, v217, v49\n\t" \
    "v_pk_add_f16 v218, v218, v50\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "v_pk_add_f16 v219, v219, v51\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "ds_read_b128 v[104:107], %[ka6] offset:8192\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_f16_f32 v160, v160, v161\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_f16_f32 v161, v162, v163\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_f16_f32 v162, v164, v165\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_cvt_pk_f16_f32 v163, v166, v167\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[128:131], a[128:131], v[64:79]\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:24576\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "ds_read_b128 v[108:111], %[ka7] offset:8192\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_f16_f32 v168, v168, v169\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v216, v216, v56\n\t" \
    "v_cvt_pk_f16_f32 v169, v170, v171\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "v_pk_add_f16 v217, v217, v57\n\t" \
    "v_pk_add_f16 v218, v218, v58\n\t" \
    "v_pk_add_f16 v219, v219, v59\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_f16_f32 v170, v172, v173\n\t" \
    "v_pk_add_f16 v216, v216, v217\n\t" \
    "v_pk_add_f16 v218, v218, v219\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v171, v174, v175\n\t" \
    "v_pk_add_f16 v216, v216, v218\n\t" \
    "v_cvt_f32_f16_e32 v221, v216\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:28672\n\t" \
    "v_cvt_f32_f16_sdwa v223, v216 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[96:99], a[144:147], v[16:31]\n\t" \
    "v_add_f32 v221, v221, v223\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[100:103], a[148:151], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[104:107], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], v[108:111], a[156:159], v[16:31]\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v176, v176, v177\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v177, v178, v179\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v178, v180, v181\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_cvt_pk_f16_f32 v179, v182, v183\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:32768\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:49152\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v184, v184, v185\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:36864\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "v_cvt_pk_f16_f32 v185, v186, v187\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v186, v188, v189\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v187, v190, v191\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:36864\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:53248\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v212, v0, v1\n\t" \
    "v_pk_add_f16 v213, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v192, v192, v193\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:40960\n\t" \
    "v_cvt_pk_f16_f32 v193, v194, v195\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v194, v196, v197\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_cvt_pk_f16_f32 v195, v198, v199\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:40960\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:57344\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v200, v200, v201\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:45056\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_cvt_pk_f16_f32 v201, v202, v203\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v202, v204, v205\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v203, v206, v207\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:45056\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:61440\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v214, v8, v9\n\t" \
    "v_pk_add_f16 v215, v10, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:32768\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[112:115], a[176:179], v[80:95]\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:0\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:32768\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:36864\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:36864\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:40960\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:40960\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:0\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:45056\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:45056\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[128:131], a[160:163], v[80:95]\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:32768\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v212, v212, v16\n\t" \
    "v_pk_add_f16 v213, v213, v17\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:32768\n\t" \
    "v_pk_add_f16 v214, v214, v18\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_pk_add_f16 v215, v215, v19\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:36864\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:36864\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:0\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:40960\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:0\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:40960\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[112:115], a[160:163], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:45056\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:45056\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[116:119], a[164:167], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:32768\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:32768\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[120:123], a[168:171], v[32:47]\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:36864\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v212, v212, v24\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:36864\n\t" \
    "v_pk_add_f16 v213, v213, v25\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], v[124:127], a[172:175], v[32:47]\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_pk_add_f16 v214, v214, v26\n\t" \
    "v_pk_add_f16 v215, v215, v27\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:40960\n\t" \
    "v_pk_add_f16 v212, v212, v213\n\t" \
    "v_pk_add_f16 v214, v214, v215\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[96:99], a[176:179], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:40960\n\t" \
    "v_pk_add_f16 v212, v212, v214\n\t" \
    "v_cvt_f32_f16_e32 v220, v212\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:45056\n\t" \
    "v_cvt_f32_f16_sdwa v222, v212 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v220, v220, v222\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[100:103], a[180:183], v[48:63]\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:45056\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[104:107], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], v[108:111], a[188:191], v[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:16384\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:16384\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:16384\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:16384\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:16384\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v216, v32, v33\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_pk_add_f16 v217, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[224:227], v[0:3], a[32:47]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:24576\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:24576\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:24576\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[240:243], v[0:3], a[48:63]\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:24576\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "v_pk_add_f16 v218, v40, v41\n\t" \
    "v_pk_add_f16 v219, v42, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v216, v216, v48\n\t" \
    "v_pk_add_f16 v217, v217, v49\n\t" \
    "v_pk_add_f16 v218, v218, v50\n\t" \
    "v_pk_add_f16 v219, v219, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v216, v216, v56\n\t" \
    "v_pk_add_f16 v217, v217, v57\n\t" \
    "v_pk_add_f16 v218, v218, v58\n\t" \
    "v_pk_add_f16 v219, v219, v59\n\t" \
    "v_pk_add_f16 v216, v216, v217\n\t" \
    "v_pk_add_f16 v218, v218, v219\n\t" \
    "v_pk_add_f16 v216, v216, v218\n\t" \
    "v_cvt_f32_f16_e32 v221, v216\n\t" \
    "v_cvt_f32_f16_sdwa v223, v216 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v221, v221, v223\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:256\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:288\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:320\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:352\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:384\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:416\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:448\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:480\n\t" \
    "ds_write_b128 %[oa], a[64:67] offset:16896\n\t" \
    "ds_write_b128 %[oa], a[68:71] offset:16928\n\t" \
    "ds_write_b128 %[oa], a[72:75] offset:16960\n\t" \
    "ds_write_b128 %[oa], a[76:79] offset:16992\n\t" \
    "ds_write_b128 %[oa], a[80:83] offset:17024\n\t" \
    "ds_write_b128 %[oa], a[84:87] offset:17056\n\t" \
    "ds_write_b128 %[oa], a[88:91] offset:17088\n\t" \
    "ds_write_b128 %[oa], a[92:95] offset:17120\n\t" \
    "ds_write_b128 %[oa], a[96:99] offset:17152\n\t" \
    "ds_write_b128 %[oa], a[100:103] offset:17184\n\t" \
    "ds_write_b128 %[oa], a[104:107] offset:17216\n\t" \
    "ds_write_b128 %[oa], a[108:111] offset:17248\n\t" \
    "ds_write_b128 %[oa], a[112:115] offset:17280\n\t" \
    "ds_write_b128 %[oa], a[116:119] offset:17312\n\t" \
    "ds_write_b128 %[oa], a[120:123] offset:17344\n\t" \
    "ds_write_b128 %[oa], a[124:127] offset:17376\n\t" \
    "v_mov_b32 %[om0], v208\n\t" \
    "v_mov_b32 %[ol0], v210\n\t" \
    "v_mov_b32 %[om1], v209\n\t" \
    "v_mov_b32 %[ol1], v211\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS_ASM_D128_BF16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v210, 0\n\t" \
    "v_mov_b32 v211, 0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "v_add_u32 v4, %[qb], %[ka4]\n\t" \
    "v_add_u32 v5, %[qb], %[ka5]\n\t" \
    "v_add_u32 v6, %[qb], %[ka6]\n\t" \
    "v_add_u32 v7, %[qb], %[ka7]\n\t" \
    "ds_read_b128 a[128:131], v0 offset:0\n\t" \
    "ds_read_b128 a[132:135], v1 offset:0\n\t" \
    "ds_read_b128 a[136:139], v2 offset:0\n\t" \
    "ds_read_b128 a[140:143], v3 offset:0\n\t" \
    "ds_read_b128 a[144:147], v4 offset:0\n\t" \
    "ds_read_b128 a[148:151], v5 offset:0\n\t" \
    "ds_read_b128 a[152:155], v6 offset:0\n\t" \
    "ds_read_b128 a[156:159], v7 offset:0\n\t" \
    "ds_read_b128 a[160:163], v0 offset:8192\n\t" \
    "ds_read_b128 a[164:167], v1 offset:8192\n\t" \
    "ds_read_b128 a[168:171], v2 offset:8192\n\t" \
    "ds_read_b128 a[172:175], v3 offset:8192\n\t" \
    "ds_read_b128 a[176:179], v4 offset:8192\n\t" \
    "ds_read_b128 a[180:183], v5 offset:8192\n\t" \
    "ds_read_b128 a[184:187], v6 offset:8192\n\t" \
    "ds_read_b128 a[188:191], v7 offset:8192\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:0\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:0\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:0\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:0\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:8192\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:8192\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:8192\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:8192\n\t" \
    "ds_read_b128 v[64:67], %[ka4] offset:8192\n\t" \
    "ds_read_b128 v[68:71], %[ka5] offset:8192\n\t" \
    "ds_read_b128 v[72:75], %[ka6] offset:8192\n\t" \
    "ds_read_b128 v[76:79], %[ka7] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[128:131], 0\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(13)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[128:131], a[128:131], 0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[64:67], a[144:147], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[68:71], a[148:151], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[72:75], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[76:79], a[156:159], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[96:99], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[100:103], a[164:167], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[104:107], a[168:171], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[108:111], a[172:175], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[112:115], a[176:179], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[128:131], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[64:67], a[176:179], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[68:71], a[180:183], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[72:75], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[76:79], a[188:191], v[48:63]\n\t" \
    "v_max3_f32 v208, v0, v1, v2\n\t" \
    "v_max3_f32 v208, v208, v3, v4\n\t" \
    "v_max3_f32 v208, v208, v5, v6\n\t" \
    "v_max3_f32 v208, v208, v7, v8\n\t" \
    "v_max3_f32 v208, v208, v9, v10\n\t" \
    "v_max3_f32 v208, v208, v11, v12\n\t" \
    "v_max3_f32 v208, v208, v13, v14\n\t" \
    "v_max3_f32 v208, v208, v15, v16\n\t" \
    "v_max3_f32 v208, v208, v17, v18\n\t" \
    "v_max3_f32 v208, v208, v19, v20\n\t" \
    "v_max3_f32 v208, v208, v21, v22\n\t" \
    "v_max3_f32 v208, v208, v23, v24\n\t" \
    "v_max3_f32 v208, v208, v25, v26\n\t" \
    "v_max3_f32 v208, v208, v27, v28\n\t" \
    "v_max3_f32 v208, v208, v29, v30\n\t" \
    "v_max_f32 v208, v208, v31\n\t" \
    "v_mov_b32 v222, v208\n\t" \
    "v_mov_b32 v223, v208\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v222, v223\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v208, v222, v223\n\t" \
    "v_max3_f32 v209, v32, v33, v34\n\t" \
    "v_max3_f32 v209, v209, v35, v36\n\t" \
    "v_max3_f32 v209, v209, v37, v38\n\t" \
    "v_max3_f32 v209, v209, v39, v40\n\t" \
    "v_max3_f32 v209, v209, v41, v42\n\t" \
    "v_max3_f32 v209, v209, v43, v44\n\t" \
    "v_max3_f32 v209, v209, v45, v46\n\t" \
    "v_max3_f32 v209, v209, v47, v48\n\t" \
    "v_max3_f32 v209, v209, v49, v50\n\t" \
    "v_max3_f32 v209, v209, v51, v52\n\t" \
    "v_max3_f32 v209, v209, v53, v54\n\t" \
    "v_max3_f32 v209, v209, v55, v56\n\t" \
    "v_max3_f32 v209, v209, v57, v58\n\t" \
    "v_max3_f32 v209, v209, v59, v60\n\t" \
    "v_max3_f32 v209, v209, v61, v62\n\t" \
    "v_max_f32 v209, v209, v63\n\t" \
    "v_mov_b32 v222, v209\n\t" \
    "v_mov_b32 v223, v209\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v222, v223\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v209, v222, v223\n\t" \
    "v_sub_f32 v64, 0, v208\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v208\n\t" \
    "v_sub_f32 v1, v1, v208\n\t" \
    "v_sub_f32 v2, v2, v208\n\t" \
    "v_sub_f32 v3, v3, v208\n\t" \
    "v_sub_f32 v4, v4, v208\n\t" \
    "v_sub_f32 v5, v5, v208\n\t" \
    "v_sub_f32 v6, v6, v208\n\t" \
    "v_sub_f32 v7, v7, v208\n\t" \
    "v_sub_f32 v8, v8, v208\n\t" \
    "v_sub_f32 v9, v9, v208\n\t" \
    "v_sub_f32 v10, v10, v208\n\t" \
    "v_sub_f32 v11, v11, v208\n\t" \
    "v_sub_f32 v12, v12, v208\n\t" \
    "v_sub_f32 v13, v13, v208\n\t" \
    "v_sub_f32 v14, v14, v208\n\t" \
    "v_sub_f32 v15, v15, v208\n\t" \
    "v_sub_f32 v16, v16, v208\n\t" \
    "v_sub_f32 v17, v17, v208\n\t" \
    "v_sub_f32 v18, v18, v208\n\t" \
    "v_sub_f32 v19, v19, v208\n\t" \
    "v_sub_f32 v20, v20, v208\n\t" \
    "v_sub_f32 v21, v21, v208\n\t" \
    "v_sub_f32 v22, v22, v208\n\t" \
    "v_sub_f32 v23, v23, v208\n\t" \
    "v_sub_f32 v24, v24, v208\n\t" \
    "v_sub_f32 v25, v25, v208\n\t" \
    "v_sub_f32 v26, v26, v208\n\t" \
    "v_sub_f32 v27, v27, v208\n\t" \
    "v_sub_f32 v28, v28, v208\n\t" \
    "v_sub_f32 v29, v29, v208\n\t" \
    "v_sub_f32 v30, v30, v208\n\t" \
    "v_sub_f32 v31, v31, v208\n\t" \
    "v_sub_f32 v80, 0, v209\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v209\n\t" \
    "v_sub_f32 v33, v33, v209\n\t" \
    "v_sub_f32 v34, v34, v209\n\t" \
    "v_sub_f32 v35, v35, v209\n\t" \
    "v_sub_f32 v36, v36, v209\n\t" \
    "v_sub_f32 v37, v37, v209\n\t" \
    "v_sub_f32 v38, v38, v209\n\t" \
    "v_sub_f32 v39, v39, v209\n\t" \
    "v_sub_f32 v40, v40, v209\n\t" \
    "v_sub_f32 v41, v41, v209\n\t" \
    "v_sub_f32 v42, v42, v209\n\t" \
    "v_sub_f32 v43, v43, v209\n\t" \
    "v_sub_f32 v44, v44, v209\n\t" \
    "v_sub_f32 v45, v45, v209\n\t" \
    "v_sub_f32 v46, v46, v209\n\t" \
    "v_sub_f32 v47, v47, v209\n\t" \
    "v_sub_f32 v48, v48, v209\n\t" \
    "v_sub_f32 v49, v49, v209\n\t" \
    "v_sub_f32 v50, v50, v209\n\t" \
    "v_sub_f32 v51, v51, v209\n\t" \
    "v_sub_f32 v52, v52, v209\n\t" \
    "v_sub_f32 v53, v53, v209\n\t" \
    "v_sub_f32 v54, v54, v209\n\t" \
    "v_sub_f32 v55, v55, v209\n\t" \
    "v_sub_f32 v56, v56, v209\n\t" \
    "v_sub_f32 v57, v57, v209\n\t" \
    "v_sub_f32 v58, v58, v209\n\t" \
    "v_sub_f32 v59, v59, v209\n\t" \
    "v_sub_f32 v60, v60, v209\n\t" \
    "v_sub_f32 v61, v61, v209\n\t" \
    "v_sub_f32 v62, v62, v209\n\t" \
    "v_sub_f32 v63, v63, v209\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v212, v0, v4\n\t" \
    "v_add_f32 v213, v1, v5\n\t" \
    "v_add_f32 v214, v2, v6\n\t" \
    "v_add_f32 v215, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v212, v212, v8\n\t" \
    "v_add_f32 v212, v212, v12\n\t" \
    "v_add_f32 v213, v213, v9\n\t" \
    "v_add_f32 v213, v213, v13\n\t" \
    "v_add_f32 v214, v214, v10\n\t" \
    "v_add_f32 v214, v214, v14\n\t" \
    "v_add_f32 v215, v215, v11\n\t" \
    "v_add_f32 v215, v215, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v212, v212, v16\n\t" \
    "v_add_f32 v212, v212, v20\n\t" \
    "v_add_f32 v213, v213, v17\n\t" \
    "v_add_f32 v213, v213, v21\n\t" \
    "v_add_f32 v214, v214, v18\n\t" \
    "v_add_f32 v214, v214, v22\n\t" \
    "v_add_f32 v215, v215, v19\n\t" \
    "v_add_f32 v215, v215, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v212, v212, v24\n\t" \
    "v_add_f32 v212, v212, v28\n\t" \
    "v_add_f32 v213, v213, v25\n\t" \
    "v_add_f32 v213, v213, v29\n\t" \
    "v_add_f32 v214, v214, v26\n\t" \
    "v_add_f32 v214, v214, v30\n\t" \
    "v_add_f32 v215, v215, v27\n\t" \
    "v_add_f32 v215, v215, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v212, v212, v213\n\t" \
    "v_add_f32 v214, v214, v215\n\t" \
    "v_add_f32 v220, v212, v214\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v216, v32, v36\n\t" \
    "v_add_f32 v217, v33, v37\n\t" \
    "v_add_f32 v218, v34, v38\n\t" \
    "v_add_f32 v219, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v216, v216, v40\n\t" \
    "v_add_f32 v216, v216, v44\n\t" \
    "v_add_f32 v217, v217, v41\n\t" \
    "v_add_f32 v217, v217, v45\n\t" \
    "v_add_f32 v218, v218, v42\n\t" \
    "v_add_f32 v218, v218, v46\n\t" \
    "v_add_f32 v219, v219, v43\n\t" \
    "v_add_f32 v219, v219, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:32768\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:36864\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:40960\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:45056\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:45056\n\t" \
    "v_accvgpr_write_b32 a64, 0\n\t" \
    "v_accvgpr_write_b32 a65, 0\n\t" \
    "v_accvgpr_write_b32 a66, 0\n\t" \
    "v_accvgpr_write_b32 a67, 0\n\t" \
    "v_accvgpr_write_b32 a68, 0\n\t" \
    "v_accvgpr_write_b32 a69, 0\n\t" \
    "v_accvgpr_write_b32 a70, 0\n\t" \
    "v_accvgpr_write_b32 a71, 0\n\t" \
    "v_accvgpr_write_b32 a72, 0\n\t" \
    "v_accvgpr_write_b32 a73, 0\n\t" \
    "v_accvgpr_write_b32 a74, 0\n\t" \
    "v_accvgpr_write_b32 a75, 0\n\t" \
    "v_accvgpr_write_b32 a76, 0\n\t" \
    "v_accvgpr_write_b32 a77, 0\n\t" \
    "v_accvgpr_write_b32 a78, 0\n\t" \
    "v_accvgpr_write_b32 a79, 0\n\t" \
    "v_accvgpr_write_b32 a80, 0\n\t" \
    "v_accvgpr_write_b32 a81, 0\n\t" \
    "v_accvgpr_write_b32 a82, 0\n\t" \
    "v_accvgpr_write_b32 a83, 0\n\t" \
    "v_accvgpr_write_b32 a84, 0\n\t" \
    "v_accvgpr_write_b32 a85, 0\n\t" \
    "v_accvgpr_write_b32 a86, 0\n\t" \
    "v_accvgpr_write_b32 a87, 0\n\t" \
    "v_accvgpr_write_b32 a88, 0\n\t" \
    "v_accvgpr_write_b32 a89, 0\n\t" \
    "v_accvgpr_write_b32 a90, 0\n\t" \
    "v_accvgpr_write_b32 a91, 0\n\t" \
    "v_accvgpr_write_b32 a92, 0\n\t" \
    "v_accvgpr_write_b32 a93, 0\n\t" \
    "v_accvgpr_write_b32 a94, 0\n\t" \
    "v_accvgpr_write_b32 a95, 0\n\t" \
    "v_accvgpr_write_b32 a96, 0\n\t" \
    "v_accvgpr_write_b32 a97, 0\n\t" \
    "v_accvgpr_write_b32 a98, 0\n\t" \
    "v_accvgpr_write_b32 a99, 0\n\t" \
    "v_accvgpr_write_b32 a100, 0\n\t" \
    "v_accvgpr_write_b32 a101, 0\n\t" \
    "v_accvgpr_write_b32 a102, 0\n\t" \
    "v_accvgpr_write_b32 a103, 0\n\t" \
    "v_accvgpr_write_b32 a104, 0\n\t" \
    "v_accvgpr_write_b32 a105, 0\n\t" \
    "v_accvgpr_write_b32 a106, 0\n\t" \
    "v_accvgpr_write_b32 a107, 0\n\t" \
    "v_accvgpr_write_b32 a108, 0\n\t" \
    "v_accvgpr_write_b32 a109, 0\n\t" \
    "v_accvgpr_write_b32 a110, 0\n\t" \
    "v_accvgpr_write_b32 a111, 0\n\t" \
    "v_accvgpr_write_b32 a112, 0\n\t" \
    "v_accvgpr_write_b32 a113, 0\n\t" \
    "v_accvgpr_write_b32 a114, 0\n\t" \
    "v_accvgpr_write_b32 a115, 0\n\t" \
    "v_accvgpr_write_b32 a116, 0\n\t" \
    "v_accvgpr_write_b32 a117, 0\n\t" \
    "v_accvgpr_write_b32 a118, 0\n\t" \
    "v_accvgpr_write_b32 a119, 0\n\t" \
    "v_accvgpr_write_b32 a120, 0\n\t" \
    "v_accvgpr_write_b32 a121, 0\n\t" \
    "v_accvgpr_write_b32 a122, 0\n\t" \
    "v_accvgpr_write_b32 a123, 0\n\t" \
    "v_accvgpr_write_b32 a124, 0\n\t" \
    "v_accvgpr_write_b32 a125, 0\n\t" \
    "v_accvgpr_write_b32 a126, 0\n\t" \
    "v_accvgpr_write_b32 a127, 0\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[224:227], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[240:243], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_bf16_f32 v160, v160, v161\n\t" \
    "v_cvt_pk_bf16_f32 v161, v162, v163\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_bf16_f32 v162, v164, v165\n\t" \
    "v_cvt_pk_bf16_f32 v163, v166, v167\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:24576\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_bf16_f32 v168, v168, v169\n\t" \
    "v_cvt_pk_bf16_f32 v169, v170, v171\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_bf16_f32 v170, v172, v173\n\t" \
    "v_cvt_pk_bf16_f32 v171, v174, v175\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:28672\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v176, v176, v177\n\t" \
    "v_cvt_pk_bf16_f32 v177, v178, v179\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v178, v180, v181\n\t" \
    "v_cvt_pk_bf16_f32 v179, v182, v183\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:49152\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v184, v184, v185\n\t" \
    "v_cvt_pk_bf16_f32 v185, v186, v187\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v186, v188, v189\n\t" \
    "v_cvt_pk_bf16_f32 v187, v190, v191\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:53248\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v192, v192, v193\n\t" \
    "v_cvt_pk_bf16_f32 v193, v194, v195\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_bf16_f32 v194, v196, v197\n\t" \
    "v_cvt_pk_bf16_f32 v195, v198, v199\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:57344\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_bf16_f32 v200, v200, v201\n\t" \
    "v_cvt_pk_bf16_f32 v201, v202, v203\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_bf16_f32 v202, v204, v205\n\t" \
    "v_cvt_pk_bf16_f32 v203, v206, v207\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:61440\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:16384\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:16384\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:16384\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:16384\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:16384\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:16384\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:16384\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:16384\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:24576\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:24576\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:24576\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:24576\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[128:131], v[64:79]\n\t" \
    "ds_read_b128 v[96:99], %[ka4] offset:24576\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "ds_read_b128 v[100:103], %[ka5] offset:24576\n\t" \
    "v_add_f32 v216, v216, v48\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "v_add_f32 v216, v216, v52\n\t" \
    "v_add_f32 v217, v217, v49\n\t" \
    "v_add_f32 v217, v217, v53\n\t" \
    "v_add_f32 v218, v218, v50\n\t" \
    "v_add_f32 v218, v218, v54\n\t" \
    "v_add_f32 v219, v219, v51\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:0\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_add_f32 v219, v219, v55\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:4096\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "ds_read_b128 v[104:107], %[ka6] offset:24576\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_bf16_f32 v160, v160, v161\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v161, v162, v163\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_bf16_f32 v162, v164, v165\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[128:131], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_cvt_pk_bf16_f32 v163, v166, v167\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v216, v216, v56\n\t" \
    "v_add_f32 v216, v216, v60\n\t" \
    "v_add_f32 v217, v217, v57\n\t" \
    "ds_read_b128 v[108:111], %[ka7] offset:24576\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_bf16_f32 v168, v168, v169\n\t" \
    "v_add_f32 v217, v217, v61\n\t" \
    "v_add_f32 v218, v218, v58\n\t" \
    "v_cvt_pk_bf16_f32 v169, v170, v171\n\t" \
    "v_add_f32 v218, v218, v62\n\t" \
    "v_add_f32 v219, v219, v59\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "v_add_f32 v219, v219, v63\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_bf16_f32 v170, v172, v173\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v171, v174, v175\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[96:99], a[144:147], v[16:31]\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v216, v216, v217\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:12288\n\t" \
    "v_add_f32 v218, v218, v219\n\t" \
    "v_add_f32 v221, v216, v218\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[100:103], a[148:151], v[16:31]\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[104:107], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[108:111], a[156:159], v[16:31]\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v176, v176, v177\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "v_cvt_pk_bf16_f32 v177, v178, v179\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v178, v180, v181\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:49152\n\t" \
    "v_cvt_pk_bf16_f32 v179, v182, v183\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:49152\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:32768\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v184, v184, v185\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:53248\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_bf16_f32 v185, v186, v187\n\t" \
    "v_add_f32 v212, v0, v4\n\t" \
    "v_add_f32 v213, v1, v5\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v186, v188, v189\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_add_f32 v214, v2, v6\n\t" \
    "v_add_f32 v215, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v187, v190, v191\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:53248\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:36864\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v192, v192, v193\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:57344\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_cvt_pk_bf16_f32 v193, v194, v195\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v194, v196, v197\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_cvt_pk_bf16_f32 v195, v198, v199\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:57344\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:40960\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v200, v200, v201\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:61440\n\t" \
    "v_add_f32 v212, v212, v8\n\t" \
    "v_add_f32 v212, v212, v12\n\t" \
    "v_cvt_pk_bf16_f32 v201, v202, v203\n\t" \
    "v_add_f32 v213, v213, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_add_f32 v213, v213, v13\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v202, v204, v205\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "v_add_f32 v214, v214, v10\n\t" \
    "v_add_f32 v214, v214, v14\n\t" \
    "v_cvt_pk_bf16_f32 v203, v206, v207\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:61440\n\t" \
    "v_add_f32 v215, v215, v11\n\t" \
    "v_add_f32 v215, v215, v15\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:45056\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:49152\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[112:115], a[176:179], v[80:95]\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:49152\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:53248\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:53248\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:57344\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:57344\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:61440\n\t" \
    "v_add_f32 v212, v212, v16\n\t" \
    "v_add_f32 v212, v212, v20\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:61440\n\t" \
    "v_add_f32 v213, v213, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[128:131], a[160:163], v[80:95]\n\t" \
    "v_add_f32 v213, v213, v21\n\t" \
    "v_add_f32 v214, v214, v18\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:49152\n\t" \
    "v_add_f32 v214, v214, v22\n\t" \
    "v_add_f32 v215, v215, v19\n\t" \
    "v_add_f32 v215, v215, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:49152\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:53248\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:16384\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:53248\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:57344\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:57344\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[112:115], a[160:163], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:61440\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[116:119], a[164:167], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:61440\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:49152\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[120:123], a[168:171], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:49152\n\t" \
    "v_add_f32 v212, v212, v24\n\t" \
    "v_add_f32 v212, v212, v28\n\t" \
    "v_add_f32 v213, v213, v25\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:53248\n\t" \
    "v_add_f32 v213, v213, v29\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[124:127], a[172:175], v[32:47]\n\t" \
    "v_add_f32 v214, v214, v26\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:53248\n\t" \
    "v_add_f32 v214, v214, v30\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_add_f32 v215, v215, v27\n\t" \
    "v_add_f32 v215, v215, v31\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[96:99], a[176:179], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:57344\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:57344\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[100:103], a[180:183], v[48:63]\n\t" \
    "v_add_f32 v212, v212, v213\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:61440\n\t" \
    "v_add_f32 v214, v214, v215\n\t" \
    "v_add_f32 v220, v212, v214\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:61440\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[104:107], a[184:187], v[48:63]\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[108:111], a[188:191], v[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:0\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:0\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:0\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:0\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_add_f32 v216, v32, v36\n\t" \
    "v_add_f32 v217, v33, v37\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:0\n\t" \
    "v_add_f32 v218, v34, v38\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_add_f32 v219, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:0\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:0\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:0\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[224:227], v[0:3], a[32:47]\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:8192\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:8192\n\t" \
    "v_add_f32 v216, v216, v40\n\t" \
    "v_add_f32 v216, v216, v44\n\t" \
    "v_add_f32 v217, v217, v41\n\t" \
    "v_add_f32 v217, v217, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:8192\n\t" \
    "v_add_f32 v218, v218, v42\n\t" \
    "v_add_f32 v218, v218, v46\n\t" \
    "v_add_f32 v219, v219, v43\n\t" \
    "v_add_f32 v219, v219, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:8192\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[240:243], v[0:3], a[48:63]\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[96:99], a[128:131], v[64:79]\n\t" \
    "ds_read_b128 v[96:99], %[ka4] offset:8192\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[132:135], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "ds_read_b128 v[100:103], %[ka5] offset:8192\n\t" \
    "v_add_f32 v216, v216, v48\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[104:107], a[136:139], v[0:15]\n\t" \
    "v_add_f32 v216, v216, v52\n\t" \
    "v_add_f32 v217, v217, v49\n\t" \
    "v_add_f32 v217, v217, v53\n\t" \
    "v_add_f32 v218, v218, v50\n\t" \
    "v_add_f32 v218, v218, v54\n\t" \
    "v_add_f32 v219, v219, v51\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[108:111], a[140:143], v[0:15]\n\t" \
    "s_waitcnt vmcnt(15)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(14)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[112:115], a[144:147], v[0:15]\n\t" \
    "s_waitcnt vmcnt(13)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(12)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_add_f32 v219, v219, v55\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[116:119], a[148:151], v[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[120:123], a[152:155], v[0:15]\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "ds_read_b128 v[104:107], %[ka6] offset:8192\n\t" \
    "s_waitcnt vmcnt(11)\n\t" \
    "v_cvt_pk_bf16_f32 v160, v160, v161\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "s_waitcnt lgkmcnt(9)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], v[124:127], a[156:159], v[0:15]\n\t" \
    "v_cvt_pk_bf16_f32 v161, v162, v163\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(10)\n\t" \
    "v_cvt_pk_bf16_f32 v162, v164, v165\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[128:131], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_cvt_pk_bf16_f32 v163, v166, v167\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "ds_write_b128 %[lo], v[160:163] offset:24576\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[132:135], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v216, v216, v56\n\t" \
    "v_add_f32 v216, v216, v60\n\t" \
    "v_add_f32 v217, v217, v57\n\t" \
    "ds_read_b128 v[108:111], %[ka7] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[136:139], a[136:139], v[16:31]\n\t" \
    "s_waitcnt vmcnt(9)\n\t" \
    "v_cvt_pk_bf16_f32 v168, v168, v169\n\t" \
    "v_add_f32 v217, v217, v61\n\t" \
    "v_add_f32 v218, v218, v58\n\t" \
    "v_cvt_pk_bf16_f32 v169, v170, v171\n\t" \
    "v_add_f32 v218, v218, v62\n\t" \
    "v_add_f32 v219, v219, v59\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[140:143], a[140:143], v[16:31]\n\t" \
    "v_add_f32 v219, v219, v63\n\t" \
    "s_waitcnt vmcnt(8)\n\t" \
    "v_cvt_pk_bf16_f32 v170, v172, v173\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v171, v174, v175\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[96:99], a[144:147], v[16:31]\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v216, v216, v217\n\t" \
    "ds_write_b128 %[lo], v[168:171] offset:28672\n\t" \
    "v_add_f32 v218, v218, v219\n\t" \
    "v_add_f32 v221, v216, v218\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[100:103], a[148:151], v[16:31]\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[104:107], a[152:155], v[16:31]\n\t" \
    "s_waitcnt lgkmcnt(1)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], v[108:111], a[156:159], v[16:31]\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v176, v176, v177\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "v_cvt_pk_bf16_f32 v177, v178, v179\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v178, v180, v181\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:32768\n\t" \
    "v_cvt_pk_bf16_f32 v179, v182, v183\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:32768\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "ds_write_b128 %[lo], v[176:179] offset:49152\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v184, v184, v185\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:36864\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_bf16_f32 v185, v186, v187\n\t" \
    "v_add_f32 v212, v0, v4\n\t" \
    "v_add_f32 v213, v1, v5\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v186, v188, v189\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_add_f32 v214, v2, v6\n\t" \
    "v_add_f32 v215, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v187, v190, v191\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:36864\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "ds_write_b128 %[lo], v[184:187] offset:53248\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v192, v192, v193\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:40960\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_cvt_pk_bf16_f32 v193, v194, v195\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v194, v196, v197\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_cvt_pk_bf16_f32 v195, v198, v199\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:40960\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "ds_write_b128 %[lo], v[192:195] offset:57344\n\t" \
    "buffer_load_dwordx4 v[160:163], %[vo2], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v200, v200, v201\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:45056\n\t" \
    "v_add_f32 v212, v212, v8\n\t" \
    "v_add_f32 v212, v212, v12\n\t" \
    "v_cvt_pk_bf16_f32 v201, v202, v203\n\t" \
    "v_add_f32 v213, v213, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_add_f32 v213, v213, v13\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v202, v204, v205\n\t" \
    "buffer_load_dwordx4 v[164:167], %[vo2], %[rsk], %[goff] offen offset:16\n\t" \
    "v_add_f32 v214, v214, v10\n\t" \
    "v_add_f32 v214, v214, v14\n\t" \
    "v_cvt_pk_bf16_f32 v203, v206, v207\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:45056\n\t" \
    "v_add_f32 v215, v215, v11\n\t" \
    "v_add_f32 v215, v215, v15\n\t" \
    "ds_write_b128 %[lo], v[200:203] offset:61440\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:32768\n\t" \
    "buffer_load_dwordx4 v[168:171], %[vo3], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[112:115], a[176:179], v[80:95]\n\t" \
    "ds_read_b128 v[112:115], %[ka0] offset:0\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:32768\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:36864\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[116:119], a[180:183], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:36864\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:40960\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[120:123], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "buffer_load_dwordx4 v[172:175], %[vo3], %[rsk], %[goff] offen offset:16\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:40960\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[124:127], a[188:191], v[32:47]\n\t" \
    "ds_read_b128 v[116:119], %[ka1] offset:0\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:45056\n\t" \
    "v_add_f32 v212, v212, v16\n\t" \
    "v_add_f32 v212, v212, v20\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:45056\n\t" \
    "v_add_f32 v213, v213, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[128:131], a[160:163], v[80:95]\n\t" \
    "v_add_f32 v213, v213, v21\n\t" \
    "v_add_f32 v214, v214, v18\n\t" \
    "ds_read_b64_tr_b16 a[224:225], %[va2_0] offset:32768\n\t" \
    "v_add_f32 v214, v214, v22\n\t" \
    "v_add_f32 v215, v215, v19\n\t" \
    "v_add_f32 v215, v215, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[132:135], a[164:167], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[226:227], %[va2_1] offset:32768\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "buffer_load_dwordx4 v[176:179], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "ds_read_b64_tr_b16 a[228:229], %[va2_0] offset:36864\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[136:139], a[168:171], v[48:63]\n\t" \
    "ds_read_b128 v[120:123], %[ka2] offset:0\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "ds_read_b64_tr_b16 a[230:231], %[va2_1] offset:36864\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[140:143], a[172:175], v[48:63]\n\t" \
    "ds_read_b128 v[124:127], %[ka3] offset:0\n\t" \
    "ds_read_b64_tr_b16 a[232:233], %[va2_0] offset:40960\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "ds_read_b64_tr_b16 a[234:235], %[va2_1] offset:40960\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[112:115], a[160:163], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[236:237], %[va2_0] offset:45056\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "buffer_load_dwordx4 v[180:183], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "s_waitcnt lgkmcnt(11)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[116:119], a[164:167], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[238:239], %[va2_1] offset:45056\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "ds_read_b64_tr_b16 a[240:241], %[va3_0] offset:32768\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[120:123], a[168:171], v[32:47]\n\t" \
    "ds_read_b64_tr_b16 a[242:243], %[va3_1] offset:32768\n\t" \
    "v_add_f32 v212, v212, v24\n\t" \
    "v_add_f32 v212, v212, v28\n\t" \
    "v_add_f32 v213, v213, v25\n\t" \
    "ds_read_b64_tr_b16 a[244:245], %[va3_0] offset:36864\n\t" \
    "v_add_f32 v213, v213, v29\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], v[124:127], a[172:175], v[32:47]\n\t" \
    "v_add_f32 v214, v214, v26\n\t" \
    "ds_read_b64_tr_b16 a[246:247], %[va3_1] offset:36864\n\t" \
    "v_add_f32 v214, v214, v30\n\t" \
    "buffer_load_dwordx4 v[184:187], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_add_f32 v215, v215, v27\n\t" \
    "v_add_f32 v215, v215, v31\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[96:99], a[176:179], v[48:63]\n\t" \
    "ds_read_b64_tr_b16 a[248:249], %[va3_0] offset:40960\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "ds_read_b64_tr_b16 a[250:251], %[va3_1] offset:40960\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[100:103], a[180:183], v[48:63]\n\t" \
    "v_add_f32 v212, v212, v213\n\t" \
    "ds_read_b64_tr_b16 a[252:253], %[va3_0] offset:45056\n\t" \
    "v_add_f32 v214, v214, v215\n\t" \
    "v_add_f32 v220, v212, v214\n\t" \
    "ds_read_b64_tr_b16 a[254:255], %[va3_1] offset:45056\n\t" \
    "v_add_f32 v210, v210, v220\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[104:107], a[184:187], v[48:63]\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v220\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], v[108:111], a[188:191], v[48:63]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 v[96:99], %[ka0] offset:16384\n\t" \
    "buffer_load_dwordx4 v[188:191], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "ds_read_b128 v[100:103], %[ka1] offset:16384\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "ds_read_b128 v[104:107], %[ka2] offset:16384\n\t" \
    "buffer_load_dwordx4 v[192:195], %[vo2], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "ds_read_b128 v[108:111], %[ka3] offset:16384\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_add_f32 v216, v32, v36\n\t" \
    "v_add_f32 v217, v33, v37\n\t" \
    "ds_read_b128 v[112:115], %[ka4] offset:16384\n\t" \
    "v_add_f32 v218, v34, v38\n\t" \
    "buffer_load_dwordx4 v[196:199], %[vo2], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_add_f32 v219, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "ds_read_b128 v[116:119], %[ka5] offset:16384\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "ds_read_b128 v[120:123], %[ka6] offset:16384\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "buffer_load_dwordx4 v[200:203], %[vo3], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "ds_read_b128 v[124:127], %[ka7] offset:16384\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[224:227], v[0:3], a[32:47]\n\t" \
    "ds_read_b128 v[128:131], %[ka0] offset:24576\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "buffer_load_dwordx4 v[204:207], %[vo3], %[rsv], %[goff] offen offset:16\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[228:231], v[8:11], a[32:47]\n\t" \
    "ds_read_b128 v[132:135], %[ka1] offset:24576\n\t" \
    "v_add_f32 v216, v216, v40\n\t" \
    "v_add_f32 v216, v216, v44\n\t" \
    "v_add_f32 v217, v217, v41\n\t" \
    "v_add_f32 v217, v217, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[232:235], v[16:19], a[32:47]\n\t" \
    "ds_read_b128 v[136:139], %[ka2] offset:24576\n\t" \
    "v_add_f32 v218, v218, v42\n\t" \
    "v_add_f32 v218, v218, v46\n\t" \
    "v_add_f32 v219, v219, v43\n\t" \
    "v_add_f32 v219, v219, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[236:239], v[24:27], a[32:47]\n\t" \
    "s_add_u32 %[goff], %[goff], 32768\n\t" \
    "ds_read_b128 v[140:143], %[ka3] offset:24576\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[240:243], v[0:3], a[48:63]\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[244:247], v[8:11], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[248:251], v[16:19], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[252:255], v[24:27], a[48:63]\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v216, v216, v48\n\t" \
    "v_add_f32 v216, v216, v52\n\t" \
    "v_add_f32 v217, v217, v49\n\t" \
    "v_add_f32 v217, v217, v53\n\t" \
    "v_add_f32 v218, v218, v50\n\t" \
    "v_add_f32 v218, v218, v54\n\t" \
    "v_add_f32 v219, v219, v51\n\t" \
    "v_add_f32 v219, v219, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v216, v216, v56\n\t" \
    "v_add_f32 v216, v216, v60\n\t" \
    "v_add_f32 v217, v217, v57\n\t" \
    "v_add_f32 v217, v217, v61\n\t" \
    "v_add_f32 v218, v218, v58\n\t" \
    "v_add_f32 v218, v218, v62\n\t" \
    "v_add_f32 v219, v219, v59\n\t" \
    "v_add_f32 v219, v219, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v216, v216, v217\n\t" \
    "v_add_f32 v218, v218, v219\n\t" \
    "v_add_f32 v221, v216, v218\n\t" \
    "v_add_f32 v211, v211, v221\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v221\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[32:35], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[40:43], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[48:51], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[56:59], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[32:35], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[40:43], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[48:51], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[56:59], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[224:227], v[32:35], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[228:231], v[40:43], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[232:235], v[48:51], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[236:239], v[56:59], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[240:243], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[244:247], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[248:251], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[252:255], v[56:59], a[112:127]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:256\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:288\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:320\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:352\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:384\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:416\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:448\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:480\n\t" \
    "ds_write_b128 %[oa], a[64:67] offset:16896\n\t" \
    "ds_write_b128 %[oa], a[68:71] offset:16928\n\t" \
    "ds_write_b128 %[oa], a[72:75] offset:16960\n\t" \
    "ds_write_b128 %[oa], a[76:79] offset:16992\n\t" \
    "ds_write_b128 %[oa], a[80:83] offset:17024\n\t" \
    "ds_write_b128 %[oa], a[84:87] offset:17056\n\t" \
    "ds_write_b128 %[oa], a[88:91] offset:17088\n\t" \
    "ds_write_b128 %[oa], a[92:95] offset:17120\n\t" \
    "ds_write_b128 %[oa], a[96:99] offset:17152\n\t" \
    "ds_write_b128 %[oa], a[100:103] offset:17184\n\t" \
    "ds_write_b128 %[oa], a[104:107] offset:17216\n\t" \
    "ds_write_b128 %[oa], a[108:111] offset:17248\n\t" \
    "ds_write_b128 %[oa], a[112:115] offset:17280\n\t" \
    "ds_write_b128 %[oa], a[116:119] offset:17312\n\t" \
    "ds_write_b128 %[oa], a[120:123] offset:17344\n\t" \
    "ds_write_b128 %[oa], a[124:127] offset:17376\n\t" \
    "v_mov_b32 %[om0], v208\n\t" \
    "v_mov_b32 %[ol0], v210\n\t" \
    "v_mov_b32 %[om1], v209\n\t" \
    "v_mov_b32 %[ol1], v211\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS_OUTPUTS_D128 [om0] "=&v"(hs_m0), [om1] "=&v"(hs_m1), [ol0] "=&v"(hs_l0), [ol1] "=&v"(hs_l1), [flg] "=&s"(hs_flag), [cnt] "+s"(hs_cnt), [goff] "+s"(hs_goff)
#define FA2_HS_INPUTS_D128 [ka0] "v"(hs_ka[0]), [ka1] "v"(hs_ka[1]), [ka2] "v"(hs_ka[2]), [ka3] "v"(hs_ka[3]), [ka4] "v"(hs_ka[4]), [ka5] "v"(hs_ka[5]), [ka6] "v"(hs_ka[6]), [ka7] "v"(hs_ka[7]), [va0_0] "v"(hs_va[0][0]), [va0_1] "v"(hs_va[0][1]), [va1_0] "v"(hs_va[1][0]), [va1_1] "v"(hs_va[1][1]), [va2_0] "v"(hs_va[2][0]), [va2_1] "v"(hs_va[2][1]), [va3_0] "v"(hs_va[3][0]), [va3_1] "v"(hs_va[3][1]), [vo0] "v"(hs_vo[0]), [vo1] "v"(hs_vo[1]), [vo2] "v"(hs_vo[2]), [vo3] "v"(hs_vo[3]), [lo] "v"(hs_lo), [oa] "v"(hs_oa), [rsk] "s"(hs_rsk), [rsv] "s"(hs_rsv), [qb] "s"(hs_qb)
#define FA2_HS_CLOBBERS_D128 "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255", "vcc", "scc", "memory"
#define FA2_HS_LDS_D128 135168

#define FA2_HS4_ASM_D64_F16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v164, 0\n\t" \
    "v_mov_b32 v165, 0\n\t" \
    "v_mov_b32 v166, 0\n\t" \
    "v_mov_b32 v167, 0\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "ds_read_b128 a[128:131], v0 offset:0\n\t" \
    "ds_read_b128 a[132:135], v1 offset:0\n\t" \
    "ds_read_b128 a[136:139], v2 offset:0\n\t" \
    "ds_read_b128 a[140:143], v3 offset:0\n\t" \
    "ds_read_b128 a[144:147], v0 offset:4096\n\t" \
    "ds_read_b128 a[148:151], v1 offset:4096\n\t" \
    "ds_read_b128 a[152:155], v2 offset:4096\n\t" \
    "ds_read_b128 a[156:159], v3 offset:4096\n\t" \
    "ds_read_b128 a[160:163], v0 offset:8192\n\t" \
    "ds_read_b128 a[164:167], v1 offset:8192\n\t" \
    "ds_read_b128 a[168:171], v2 offset:8192\n\t" \
    "ds_read_b128 a[172:175], v3 offset:8192\n\t" \
    "ds_read_b128 a[176:179], v0 offset:12288\n\t" \
    "ds_read_b128 a[180:183], v1 offset:12288\n\t" \
    "ds_read_b128 a[184:187], v2 offset:12288\n\t" \
    "ds_read_b128 a[188:191], v3 offset:12288\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:0\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:0\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:0\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:0\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:4096\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:4096\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:4096\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:4096\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:22528\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[128:131], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[128:131], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v160, v0, v1, v2\n\t" \
    "v_max3_f32 v160, v160, v3, v4\n\t" \
    "v_max3_f32 v160, v160, v5, v6\n\t" \
    "v_max3_f32 v160, v160, v7, v8\n\t" \
    "v_max3_f32 v160, v160, v9, v10\n\t" \
    "v_max3_f32 v160, v160, v11, v12\n\t" \
    "v_max3_f32 v160, v160, v13, v14\n\t" \
    "v_max3_f32 v160, v160, v15, v16\n\t" \
    "v_max3_f32 v160, v160, v17, v18\n\t" \
    "v_max3_f32 v160, v160, v19, v20\n\t" \
    "v_max3_f32 v160, v160, v21, v22\n\t" \
    "v_max3_f32 v160, v160, v23, v24\n\t" \
    "v_max3_f32 v160, v160, v25, v26\n\t" \
    "v_max3_f32 v160, v160, v27, v28\n\t" \
    "v_max3_f32 v160, v160, v29, v30\n\t" \
    "v_max_f32 v160, v160, v31\n\t" \
    "v_mov_b32 v188, v160\n\t" \
    "v_mov_b32 v189, v160\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v160, v188, v189\n\t" \
    "v_sub_f32 v64, 0, v160\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v160\n\t" \
    "v_sub_f32 v1, v1, v160\n\t" \
    "v_sub_f32 v2, v2, v160\n\t" \
    "v_sub_f32 v3, v3, v160\n\t" \
    "v_sub_f32 v4, v4, v160\n\t" \
    "v_sub_f32 v5, v5, v160\n\t" \
    "v_sub_f32 v6, v6, v160\n\t" \
    "v_sub_f32 v7, v7, v160\n\t" \
    "v_sub_f32 v8, v8, v160\n\t" \
    "v_sub_f32 v9, v9, v160\n\t" \
    "v_sub_f32 v10, v10, v160\n\t" \
    "v_sub_f32 v11, v11, v160\n\t" \
    "v_sub_f32 v12, v12, v160\n\t" \
    "v_sub_f32 v13, v13, v160\n\t" \
    "v_sub_f32 v14, v14, v160\n\t" \
    "v_sub_f32 v15, v15, v160\n\t" \
    "v_sub_f32 v16, v16, v160\n\t" \
    "v_sub_f32 v17, v17, v160\n\t" \
    "v_sub_f32 v18, v18, v160\n\t" \
    "v_sub_f32 v19, v19, v160\n\t" \
    "v_sub_f32 v20, v20, v160\n\t" \
    "v_sub_f32 v21, v21, v160\n\t" \
    "v_sub_f32 v22, v22, v160\n\t" \
    "v_sub_f32 v23, v23, v160\n\t" \
    "v_sub_f32 v24, v24, v160\n\t" \
    "v_sub_f32 v25, v25, v160\n\t" \
    "v_sub_f32 v26, v26, v160\n\t" \
    "v_sub_f32 v27, v27, v160\n\t" \
    "v_sub_f32 v28, v28, v160\n\t" \
    "v_sub_f32 v29, v29, v160\n\t" \
    "v_sub_f32 v30, v30, v160\n\t" \
    "v_sub_f32 v31, v31, v160\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v168, v0, v1\n\t" \
    "v_pk_add_f16 v169, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v170, v8, v9\n\t" \
    "v_pk_add_f16 v171, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v168, v168, v16\n\t" \
    "v_pk_add_f16 v169, v169, v17\n\t" \
    "v_pk_add_f16 v170, v170, v18\n\t" \
    "v_pk_add_f16 v171, v171, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v168, v168, v24\n\t" \
    "v_pk_add_f16 v169, v169, v25\n\t" \
    "v_pk_add_f16 v170, v170, v26\n\t" \
    "v_pk_add_f16 v171, v171, v27\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v184, v168\n\t" \
    "v_cvt_f32_f16_sdwa v188, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v184, v184, v188\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[144:147], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[144:147], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v161, v32, v33, v34\n\t" \
    "v_max3_f32 v161, v161, v35, v36\n\t" \
    "v_max3_f32 v161, v161, v37, v38\n\t" \
    "v_max3_f32 v161, v161, v39, v40\n\t" \
    "v_max3_f32 v161, v161, v41, v42\n\t" \
    "v_max3_f32 v161, v161, v43, v44\n\t" \
    "v_max3_f32 v161, v161, v45, v46\n\t" \
    "v_max3_f32 v161, v161, v47, v48\n\t" \
    "v_max3_f32 v161, v161, v49, v50\n\t" \
    "v_max3_f32 v161, v161, v51, v52\n\t" \
    "v_max3_f32 v161, v161, v53, v54\n\t" \
    "v_max3_f32 v161, v161, v55, v56\n\t" \
    "v_max3_f32 v161, v161, v57, v58\n\t" \
    "v_max3_f32 v161, v161, v59, v60\n\t" \
    "v_max3_f32 v161, v161, v61, v62\n\t" \
    "v_max_f32 v161, v161, v63\n\t" \
    "v_mov_b32 v188, v161\n\t" \
    "v_mov_b32 v189, v161\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v161, v188, v189\n\t" \
    "v_sub_f32 v80, 0, v161\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v161\n\t" \
    "v_sub_f32 v33, v33, v161\n\t" \
    "v_sub_f32 v34, v34, v161\n\t" \
    "v_sub_f32 v35, v35, v161\n\t" \
    "v_sub_f32 v36, v36, v161\n\t" \
    "v_sub_f32 v37, v37, v161\n\t" \
    "v_sub_f32 v38, v38, v161\n\t" \
    "v_sub_f32 v39, v39, v161\n\t" \
    "v_sub_f32 v40, v40, v161\n\t" \
    "v_sub_f32 v41, v41, v161\n\t" \
    "v_sub_f32 v42, v42, v161\n\t" \
    "v_sub_f32 v43, v43, v161\n\t" \
    "v_sub_f32 v44, v44, v161\n\t" \
    "v_sub_f32 v45, v45, v161\n\t" \
    "v_sub_f32 v46, v46, v161\n\t" \
    "v_sub_f32 v47, v47, v161\n\t" \
    "v_sub_f32 v48, v48, v161\n\t" \
    "v_sub_f32 v49, v49, v161\n\t" \
    "v_sub_f32 v50, v50, v161\n\t" \
    "v_sub_f32 v51, v51, v161\n\t" \
    "v_sub_f32 v52, v52, v161\n\t" \
    "v_sub_f32 v53, v53, v161\n\t" \
    "v_sub_f32 v54, v54, v161\n\t" \
    "v_sub_f32 v55, v55, v161\n\t" \
    "v_sub_f32 v56, v56, v161\n\t" \
    "v_sub_f32 v57, v57, v161\n\t" \
    "v_sub_f32 v58, v58, v161\n\t" \
    "v_sub_f32 v59, v59, v161\n\t" \
    "v_sub_f32 v60, v60, v161\n\t" \
    "v_sub_f32 v61, v61, v161\n\t" \
    "v_sub_f32 v62, v62, v161\n\t" \
    "v_sub_f32 v63, v63, v161\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v172, v32, v33\n\t" \
    "v_pk_add_f16 v173, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v174, v40, v41\n\t" \
    "v_pk_add_f16 v175, v42, v43\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v172, v172, v48\n\t" \
    "v_pk_add_f16 v173, v173, v49\n\t" \
    "v_pk_add_f16 v174, v174, v50\n\t" \
    "v_pk_add_f16 v175, v175, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v172, v172, v56\n\t" \
    "v_pk_add_f16 v173, v173, v57\n\t" \
    "v_pk_add_f16 v174, v174, v58\n\t" \
    "v_pk_add_f16 v175, v175, v59\n\t" \
    "v_pk_add_f16 v172, v172, v173\n\t" \
    "v_pk_add_f16 v174, v174, v175\n\t" \
    "v_pk_add_f16 v172, v172, v174\n\t" \
    "v_cvt_f32_f16_e32 v185, v172\n\t" \
    "v_cvt_f32_f16_sdwa v189, v172 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v185, v185, v189\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[192:195], v[32:35], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[208:211], v[32:35], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v162, v0, v1, v2\n\t" \
    "v_max3_f32 v162, v162, v3, v4\n\t" \
    "v_max3_f32 v162, v162, v5, v6\n\t" \
    "v_max3_f32 v162, v162, v7, v8\n\t" \
    "v_max3_f32 v162, v162, v9, v10\n\t" \
    "v_max3_f32 v162, v162, v11, v12\n\t" \
    "v_max3_f32 v162, v162, v13, v14\n\t" \
    "v_max3_f32 v162, v162, v15, v16\n\t" \
    "v_max3_f32 v162, v162, v17, v18\n\t" \
    "v_max3_f32 v162, v162, v19, v20\n\t" \
    "v_max3_f32 v162, v162, v21, v22\n\t" \
    "v_max3_f32 v162, v162, v23, v24\n\t" \
    "v_max3_f32 v162, v162, v25, v26\n\t" \
    "v_max3_f32 v162, v162, v27, v28\n\t" \
    "v_max3_f32 v162, v162, v29, v30\n\t" \
    "v_max_f32 v162, v162, v31\n\t" \
    "v_mov_b32 v188, v162\n\t" \
    "v_mov_b32 v189, v162\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v162, v188, v189\n\t" \
    "v_sub_f32 v96, 0, v162\n\t" \
    "v_mov_b32 v97, v96\n\t" \
    "v_mov_b32 v98, v96\n\t" \
    "v_mov_b32 v99, v96\n\t" \
    "v_mov_b32 v100, v96\n\t" \
    "v_mov_b32 v101, v96\n\t" \
    "v_mov_b32 v102, v96\n\t" \
    "v_mov_b32 v103, v96\n\t" \
    "v_mov_b32 v104, v96\n\t" \
    "v_mov_b32 v105, v96\n\t" \
    "v_mov_b32 v106, v96\n\t" \
    "v_mov_b32 v107, v96\n\t" \
    "v_mov_b32 v108, v96\n\t" \
    "v_mov_b32 v109, v96\n\t" \
    "v_mov_b32 v110, v96\n\t" \
    "v_mov_b32 v111, v96\n\t" \
    "v_sub_f32 v0, v0, v162\n\t" \
    "v_sub_f32 v1, v1, v162\n\t" \
    "v_sub_f32 v2, v2, v162\n\t" \
    "v_sub_f32 v3, v3, v162\n\t" \
    "v_sub_f32 v4, v4, v162\n\t" \
    "v_sub_f32 v5, v5, v162\n\t" \
    "v_sub_f32 v6, v6, v162\n\t" \
    "v_sub_f32 v7, v7, v162\n\t" \
    "v_sub_f32 v8, v8, v162\n\t" \
    "v_sub_f32 v9, v9, v162\n\t" \
    "v_sub_f32 v10, v10, v162\n\t" \
    "v_sub_f32 v11, v11, v162\n\t" \
    "v_sub_f32 v12, v12, v162\n\t" \
    "v_sub_f32 v13, v13, v162\n\t" \
    "v_sub_f32 v14, v14, v162\n\t" \
    "v_sub_f32 v15, v15, v162\n\t" \
    "v_sub_f32 v16, v16, v162\n\t" \
    "v_sub_f32 v17, v17, v162\n\t" \
    "v_sub_f32 v18, v18, v162\n\t" \
    "v_sub_f32 v19, v19, v162\n\t" \
    "v_sub_f32 v20, v20, v162\n\t" \
    "v_sub_f32 v21, v21, v162\n\t" \
    "v_sub_f32 v22, v22, v162\n\t" \
    "v_sub_f32 v23, v23, v162\n\t" \
    "v_sub_f32 v24, v24, v162\n\t" \
    "v_sub_f32 v25, v25, v162\n\t" \
    "v_sub_f32 v26, v26, v162\n\t" \
    "v_sub_f32 v27, v27, v162\n\t" \
    "v_sub_f32 v28, v28, v162\n\t" \
    "v_sub_f32 v29, v29, v162\n\t" \
    "v_sub_f32 v30, v30, v162\n\t" \
    "v_sub_f32 v31, v31, v162\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v176, v0, v1\n\t" \
    "v_pk_add_f16 v177, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v178, v8, v9\n\t" \
    "v_pk_add_f16 v179, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v176, v176, v16\n\t" \
    "v_pk_add_f16 v177, v177, v17\n\t" \
    "v_pk_add_f16 v178, v178, v18\n\t" \
    "v_pk_add_f16 v179, v179, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v176, v176, v24\n\t" \
    "v_pk_add_f16 v177, v177, v25\n\t" \
    "v_pk_add_f16 v178, v178, v26\n\t" \
    "v_pk_add_f16 v179, v179, v27\n\t" \
    "v_pk_add_f16 v176, v176, v177\n\t" \
    "v_pk_add_f16 v178, v178, v179\n\t" \
    "v_pk_add_f16 v176, v176, v178\n\t" \
    "v_cvt_f32_f16_e32 v186, v176\n\t" \
    "v_cvt_f32_f16_sdwa v190, v176 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v186, v186, v190\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[176:179], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[176:179], 0\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v163, v32, v33, v34\n\t" \
    "v_max3_f32 v163, v163, v35, v36\n\t" \
    "v_max3_f32 v163, v163, v37, v38\n\t" \
    "v_max3_f32 v163, v163, v39, v40\n\t" \
    "v_max3_f32 v163, v163, v41, v42\n\t" \
    "v_max3_f32 v163, v163, v43, v44\n\t" \
    "v_max3_f32 v163, v163, v45, v46\n\t" \
    "v_max3_f32 v163, v163, v47, v48\n\t" \
    "v_max3_f32 v163, v163, v49, v50\n\t" \
    "v_max3_f32 v163, v163, v51, v52\n\t" \
    "v_max3_f32 v163, v163, v53, v54\n\t" \
    "v_max3_f32 v163, v163, v55, v56\n\t" \
    "v_max3_f32 v163, v163, v57, v58\n\t" \
    "v_max3_f32 v163, v163, v59, v60\n\t" \
    "v_max3_f32 v163, v163, v61, v62\n\t" \
    "v_max_f32 v163, v163, v63\n\t" \
    "v_mov_b32 v188, v163\n\t" \
    "v_mov_b32 v189, v163\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v163, v188, v189\n\t" \
    "v_sub_f32 v112, 0, v163\n\t" \
    "v_mov_b32 v113, v112\n\t" \
    "v_mov_b32 v114, v112\n\t" \
    "v_mov_b32 v115, v112\n\t" \
    "v_mov_b32 v116, v112\n\t" \
    "v_mov_b32 v117, v112\n\t" \
    "v_mov_b32 v118, v112\n\t" \
    "v_mov_b32 v119, v112\n\t" \
    "v_mov_b32 v120, v112\n\t" \
    "v_mov_b32 v121, v112\n\t" \
    "v_mov_b32 v122, v112\n\t" \
    "v_mov_b32 v123, v112\n\t" \
    "v_mov_b32 v124, v112\n\t" \
    "v_mov_b32 v125, v112\n\t" \
    "v_mov_b32 v126, v112\n\t" \
    "v_mov_b32 v127, v112\n\t" \
    "v_sub_f32 v32, v32, v163\n\t" \
    "v_sub_f32 v33, v33, v163\n\t" \
    "v_sub_f32 v34, v34, v163\n\t" \
    "v_sub_f32 v35, v35, v163\n\t" \
    "v_sub_f32 v36, v36, v163\n\t" \
    "v_sub_f32 v37, v37, v163\n\t" \
    "v_sub_f32 v38, v38, v163\n\t" \
    "v_sub_f32 v39, v39, v163\n\t" \
    "v_sub_f32 v40, v40, v163\n\t" \
    "v_sub_f32 v41, v41, v163\n\t" \
    "v_sub_f32 v42, v42, v163\n\t" \
    "v_sub_f32 v43, v43, v163\n\t" \
    "v_sub_f32 v44, v44, v163\n\t" \
    "v_sub_f32 v45, v45, v163\n\t" \
    "v_sub_f32 v46, v46, v163\n\t" \
    "v_sub_f32 v47, v47, v163\n\t" \
    "v_sub_f32 v48, v48, v163\n\t" \
    "v_sub_f32 v49, v49, v163\n\t" \
    "v_sub_f32 v50, v50, v163\n\t" \
    "v_sub_f32 v51, v51, v163\n\t" \
    "v_sub_f32 v52, v52, v163\n\t" \
    "v_sub_f32 v53, v53, v163\n\t" \
    "v_sub_f32 v54, v54, v163\n\t" \
    "v_sub_f32 v55, v55, v163\n\t" \
    "v_sub_f32 v56, v56, v163\n\t" \
    "v_sub_f32 v57, v57, v163\n\t" \
    "v_sub_f32 v58, v58, v163\n\t" \
    "v_sub_f32 v59, v59, v163\n\t" \
    "v_sub_f32 v60, v60, v163\n\t" \
    "v_sub_f32 v61, v61, v163\n\t" \
    "v_sub_f32 v62, v62, v163\n\t" \
    "v_sub_f32 v63, v63, v163\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v180, v32, v33\n\t" \
    "v_pk_add_f16 v181, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v182, v40, v41\n\t" \
    "v_pk_add_f16 v183, v42, v43\n\t" \
    "v_accvgpr_write_b32 a96, 0\n\t" \
    "v_accvgpr_write_b32 a97, 0\n\t" \
    "v_accvgpr_write_b32 a98, 0\n\t" \
    "v_accvgpr_write_b32 a99, 0\n\t" \
    "v_accvgpr_write_b32 a100, 0\n\t" \
    "v_accvgpr_write_b32 a101, 0\n\t" \
    "v_accvgpr_write_b32 a102, 0\n\t" \
    "v_accvgpr_write_b32 a103, 0\n\t" \
    "v_accvgpr_write_b32 a104, 0\n\t" \
    "v_accvgpr_write_b32 a105, 0\n\t" \
    "v_accvgpr_write_b32 a106, 0\n\t" \
    "v_accvgpr_write_b32 a107, 0\n\t" \
    "v_accvgpr_write_b32 a108, 0\n\t" \
    "v_accvgpr_write_b32 a109, 0\n\t" \
    "v_accvgpr_write_b32 a110, 0\n\t" \
    "v_accvgpr_write_b32 a111, 0\n\t" \
    "v_accvgpr_write_b32 a112, 0\n\t" \
    "v_accvgpr_write_b32 a113, 0\n\t" \
    "v_accvgpr_write_b32 a114, 0\n\t" \
    "v_accvgpr_write_b32 a115, 0\n\t" \
    "v_accvgpr_write_b32 a116, 0\n\t" \
    "v_accvgpr_write_b32 a117, 0\n\t" \
    "v_accvgpr_write_b32 a118, 0\n\t" \
    "v_accvgpr_write_b32 a119, 0\n\t" \
    "v_accvgpr_write_b32 a120, 0\n\t" \
    "v_accvgpr_write_b32 a121, 0\n\t" \
    "v_accvgpr_write_b32 a122, 0\n\t" \
    "v_accvgpr_write_b32 a123, 0\n\t" \
    "v_accvgpr_write_b32 a124, 0\n\t" \
    "v_accvgpr_write_b32 a125, 0\n\t" \
    "v_accvgpr_write_b32 a126, 0\n\t" \
    "v_accvgpr_write_b32 a127, 0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:8192\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:8192\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:8192\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:8192\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:12288\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:12288\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:12288\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:12288\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v180, v180, v48\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_pk_add_f16 v181, v181, v49\n\t" \
    "v_pk_add_f16 v182, v182, v50\n\t" \
    "v_pk_add_f16 v183, v183, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v180, v180, v56\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "v_pk_add_f16 v181, v181, v57\n\t" \
    "v_pk_add_f16 v182, v182, v58\n\t" \
    "v_pk_add_f16 v183, v183, v59\n\t" \
    "v_pk_add_f16 v180, v180, v181\n\t" \
    "v_pk_add_f16 v182, v182, v183\n\t" \
    "v_pk_add_f16 v180, v180, v182\n\t" \
    "v_cvt_f32_f16_e32 v187, v180\n\t" \
    "v_cvt_f32_f16_sdwa v191, v180 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v187, v187, v191\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v168, v0, v1\n\t" \
    "v_pk_add_f16 v169, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v170, v8, v9\n\t" \
    "v_pk_add_f16 v171, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:24576\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:26624\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:30720\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v168, v168, v16\n\t" \
    "v_pk_add_f16 v169, v169, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_pk_add_f16 v170, v170, v18\n\t" \
    "v_pk_add_f16 v171, v171, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v168, v168, v24\n\t" \
    "v_pk_add_f16 v169, v169, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "v_pk_add_f16 v170, v170, v26\n\t" \
    "v_pk_add_f16 v171, v171, v27\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v184, v168\n\t" \
    "v_cvt_f32_f16_sdwa v188, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v184, v184, v188\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v172, v32, v33\n\t" \
    "v_pk_add_f16 v173, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v174, v40, v41\n\t" \
    "v_pk_add_f16 v175, v42, v43\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_pk_add_f16 v172, v172, v48\n\t" \
    "v_pk_add_f16 v173, v173, v49\n\t" \
    "v_pk_add_f16 v174, v174, v50\n\t" \
    "v_pk_add_f16 v175, v175, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "v_pk_add_f16 v172, v172, v56\n\t" \
    "v_pk_add_f16 v173, v173, v57\n\t" \
    "v_pk_add_f16 v174, v174, v58\n\t" \
    "v_pk_add_f16 v175, v175, v59\n\t" \
    "v_pk_add_f16 v172, v172, v173\n\t" \
    "v_pk_add_f16 v174, v174, v175\n\t" \
    "v_pk_add_f16 v172, v172, v174\n\t" \
    "v_cvt_f32_f16_e32 v185, v172\n\t" \
    "v_cvt_f32_f16_sdwa v189, v172 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v185, v185, v189\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[192:195], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v176, v0, v1\n\t" \
    "v_pk_add_f16 v177, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[208:211], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v178, v8, v9\n\t" \
    "v_pk_add_f16 v179, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_pk_add_f16 v176, v176, v16\n\t" \
    "v_pk_add_f16 v177, v177, v17\n\t" \
    "v_pk_add_f16 v178, v178, v18\n\t" \
    "v_pk_add_f16 v179, v179, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "v_pk_add_f16 v176, v176, v24\n\t" \
    "v_pk_add_f16 v177, v177, v25\n\t" \
    "v_pk_add_f16 v178, v178, v26\n\t" \
    "v_pk_add_f16 v179, v179, v27\n\t" \
    "v_pk_add_f16 v176, v176, v177\n\t" \
    "v_pk_add_f16 v178, v178, v179\n\t" \
    "v_pk_add_f16 v176, v176, v178\n\t" \
    "v_cvt_f32_f16_e32 v186, v176\n\t" \
    "v_cvt_f32_f16_sdwa v190, v176 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v186, v186, v190\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:0\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:0\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:0\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[0:3], a[64:79]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:0\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:4096\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:4096\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:4096\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:4096\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v180, v32, v33\n\t" \
    "v_pk_add_f16 v181, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[0:3], a[80:95]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v182, v40, v41\n\t" \
    "v_pk_add_f16 v183, v42, v43\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_f16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_f16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_f16_f32 v130, v132, v133\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_cvt_pk_f16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v180, v180, v48\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_pk_add_f16 v181, v181, v49\n\t" \
    "v_pk_add_f16 v182, v182, v50\n\t" \
    "v_pk_add_f16 v183, v183, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_f16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_f16_f32 v137, v138, v139\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_f16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_f16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v180, v180, v56\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "v_pk_add_f16 v181, v181, v57\n\t" \
    "v_pk_add_f16 v182, v182, v58\n\t" \
    "v_pk_add_f16 v183, v183, v59\n\t" \
    "v_pk_add_f16 v180, v180, v181\n\t" \
    "v_pk_add_f16 v182, v182, v183\n\t" \
    "v_pk_add_f16 v180, v180, v182\n\t" \
    "v_cvt_f32_f16_e32 v187, v180\n\t" \
    "v_cvt_f32_f16_sdwa v191, v180 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v187, v187, v191\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_f16_f32 v144, v144, v145\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_f16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_f16_f32 v146, v148, v149\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_cvt_pk_f16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_f16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_f16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_f16_f32 v154, v156, v157\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v168, v0, v1\n\t" \
    "v_pk_add_f16 v169, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_cvt_pk_f16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v170, v8, v9\n\t" \
    "v_pk_add_f16 v171, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:16384\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:18432\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:22528\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_pk_add_f16 v168, v168, v16\n\t" \
    "v_pk_add_f16 v169, v169, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_pk_add_f16 v170, v170, v18\n\t" \
    "v_pk_add_f16 v171, v171, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_pk_add_f16 v168, v168, v24\n\t" \
    "v_pk_add_f16 v169, v169, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "v_pk_add_f16 v170, v170, v26\n\t" \
    "v_pk_add_f16 v171, v171, v27\n\t" \
    "v_pk_add_f16 v168, v168, v169\n\t" \
    "v_pk_add_f16 v170, v170, v171\n\t" \
    "v_pk_add_f16 v168, v168, v170\n\t" \
    "v_cvt_f32_f16_e32 v184, v168\n\t" \
    "v_cvt_f32_f16_sdwa v188, v168 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v184, v184, v188\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_mfma_f32_32x32x16_f16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v172, v32, v33\n\t" \
    "v_pk_add_f16 v173, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_f16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v174, v40, v41\n\t" \
    "v_pk_add_f16 v175, v42, v43\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[224:227], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_mfma_f32_32x32x16_f16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_pk_add_f16 v172, v172, v48\n\t" \
    "v_pk_add_f16 v173, v173, v49\n\t" \
    "v_pk_add_f16 v174, v174, v50\n\t" \
    "v_pk_add_f16 v175, v175, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[240:243], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_mfma_f32_32x32x16_f16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "v_pk_add_f16 v172, v172, v56\n\t" \
    "v_pk_add_f16 v173, v173, v57\n\t" \
    "v_pk_add_f16 v174, v174, v58\n\t" \
    "v_pk_add_f16 v175, v175, v59\n\t" \
    "v_pk_add_f16 v172, v172, v173\n\t" \
    "v_pk_add_f16 v174, v174, v175\n\t" \
    "v_pk_add_f16 v172, v172, v174\n\t" \
    "v_cvt_f32_f16_e32 v185, v172\n\t" \
    "v_cvt_f32_f16_sdwa v189, v172 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v185, v185, v189\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[192:195], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_cvt_pk_f16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_f16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_f16_f32 v2, v4, v5\n\t" \
    "v_mfma_f32_32x32x16_f16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_f16_f32 v3, v6, v7\n\t" \
    "v_pk_add_f16 v176, v0, v1\n\t" \
    "v_pk_add_f16 v177, v2, v3\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[208:211], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_cvt_pk_f16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_f16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_f16_f32 v10, v12, v13\n\t" \
    "v_mfma_f32_32x32x16_f16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_cvt_pk_f16_f32 v11, v14, v15\n\t" \
    "v_pk_add_f16 v178, v8, v9\n\t" \
    "v_pk_add_f16 v179, v10, v11\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[224:227], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_cvt_pk_f16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_f16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_f16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_f16_f32 v19, v22, v23\n\t" \
    "v_mfma_f32_32x32x16_f16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_pk_add_f16 v176, v176, v16\n\t" \
    "v_pk_add_f16 v177, v177, v17\n\t" \
    "v_pk_add_f16 v178, v178, v18\n\t" \
    "v_pk_add_f16 v179, v179, v19\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[240:243], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_cvt_pk_f16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_f16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_f16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_f16_f32 v27, v30, v31\n\t" \
    "v_mfma_f32_32x32x16_f16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "v_pk_add_f16 v176, v176, v24\n\t" \
    "v_pk_add_f16 v177, v177, v25\n\t" \
    "v_pk_add_f16 v178, v178, v26\n\t" \
    "v_pk_add_f16 v179, v179, v27\n\t" \
    "v_pk_add_f16 v176, v176, v177\n\t" \
    "v_pk_add_f16 v178, v178, v179\n\t" \
    "v_pk_add_f16 v176, v176, v178\n\t" \
    "v_cvt_f32_f16_e32 v186, v176\n\t" \
    "v_cvt_f32_f16_sdwa v190, v176 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v186, v186, v190\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:8192\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:8192\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:8192\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[192:195], v[0:3], a[64:79]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:8192\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:12288\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:12288\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:12288\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:12288\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_cvt_pk_f16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_f16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_f16_f32 v34, v36, v37\n\t" \
    "v_mfma_f32_32x32x16_f16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_cvt_pk_f16_f32 v35, v38, v39\n\t" \
    "v_pk_add_f16 v180, v32, v33\n\t" \
    "v_pk_add_f16 v181, v34, v35\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[208:211], v[0:3], a[80:95]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_cvt_pk_f16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_f16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_f16_f32 v42, v44, v45\n\t" \
    "v_mfma_f32_32x32x16_f16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_cvt_pk_f16_f32 v43, v46, v47\n\t" \
    "v_pk_add_f16 v182, v40, v41\n\t" \
    "v_pk_add_f16 v183, v42, v43\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_cvt_pk_f16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_f16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_f16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_f16_f32 v51, v54, v55\n\t" \
    "v_pk_add_f16 v180, v180, v48\n\t" \
    "v_pk_add_f16 v181, v181, v49\n\t" \
    "v_pk_add_f16 v182, v182, v50\n\t" \
    "v_pk_add_f16 v183, v183, v51\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_cvt_pk_f16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_f16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_f16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_f16_f32 v59, v62, v63\n\t" \
    "v_pk_add_f16 v180, v180, v56\n\t" \
    "v_pk_add_f16 v181, v181, v57\n\t" \
    "v_pk_add_f16 v182, v182, v58\n\t" \
    "v_pk_add_f16 v183, v183, v59\n\t" \
    "v_pk_add_f16 v180, v180, v181\n\t" \
    "v_pk_add_f16 v182, v182, v183\n\t" \
    "v_pk_add_f16 v180, v180, v182\n\t" \
    "v_cvt_f32_f16_e32 v187, v180\n\t" \
    "v_cvt_f32_f16_sdwa v191, v180 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1\n\t" \
    "v_add_f32 v187, v187, v191\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_f16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:8704\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:8736\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:8768\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:8800\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:8832\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:8864\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:8896\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:8928\n\t" \
    "ds_write_b128 %[oa], a[64:67] offset:17408\n\t" \
    "ds_write_b128 %[oa], a[68:71] offset:17440\n\t" \
    "ds_write_b128 %[oa], a[72:75] offset:17472\n\t" \
    "ds_write_b128 %[oa], a[76:79] offset:17504\n\t" \
    "ds_write_b128 %[oa], a[80:83] offset:17536\n\t" \
    "ds_write_b128 %[oa], a[84:87] offset:17568\n\t" \
    "ds_write_b128 %[oa], a[88:91] offset:17600\n\t" \
    "ds_write_b128 %[oa], a[92:95] offset:17632\n\t" \
    "ds_write_b128 %[oa], a[96:99] offset:26112\n\t" \
    "ds_write_b128 %[oa], a[100:103] offset:26144\n\t" \
    "ds_write_b128 %[oa], a[104:107] offset:26176\n\t" \
    "ds_write_b128 %[oa], a[108:111] offset:26208\n\t" \
    "ds_write_b128 %[oa], a[112:115] offset:26240\n\t" \
    "ds_write_b128 %[oa], a[116:119] offset:26272\n\t" \
    "ds_write_b128 %[oa], a[120:123] offset:26304\n\t" \
    "ds_write_b128 %[oa], a[124:127] offset:26336\n\t" \
    "v_mov_b32 %[om0], v160\n\t" \
    "v_mov_b32 %[ol0], v164\n\t" \
    "v_mov_b32 %[om1], v161\n\t" \
    "v_mov_b32 %[ol1], v165\n\t" \
    "v_mov_b32 %[om2], v162\n\t" \
    "v_mov_b32 %[ol2], v166\n\t" \
    "v_mov_b32 %[om3], v163\n\t" \
    "v_mov_b32 %[ol3], v167\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS4_ASM_D64_BF16 \
    "s_mov_b64 %[flg], 0\n\t" \
    "v_mov_b32 v164, 0\n\t" \
    "v_mov_b32 v165, 0\n\t" \
    "v_mov_b32 v166, 0\n\t" \
    "v_mov_b32 v167, 0\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_add_u32 v0, %[qb], %[ka0]\n\t" \
    "v_add_u32 v1, %[qb], %[ka1]\n\t" \
    "v_add_u32 v2, %[qb], %[ka2]\n\t" \
    "v_add_u32 v3, %[qb], %[ka3]\n\t" \
    "ds_read_b128 a[128:131], v0 offset:0\n\t" \
    "ds_read_b128 a[132:135], v1 offset:0\n\t" \
    "ds_read_b128 a[136:139], v2 offset:0\n\t" \
    "ds_read_b128 a[140:143], v3 offset:0\n\t" \
    "ds_read_b128 a[144:147], v0 offset:4096\n\t" \
    "ds_read_b128 a[148:151], v1 offset:4096\n\t" \
    "ds_read_b128 a[152:155], v2 offset:4096\n\t" \
    "ds_read_b128 a[156:159], v3 offset:4096\n\t" \
    "ds_read_b128 a[160:163], v0 offset:8192\n\t" \
    "ds_read_b128 a[164:167], v1 offset:8192\n\t" \
    "ds_read_b128 a[168:171], v2 offset:8192\n\t" \
    "ds_read_b128 a[172:175], v3 offset:8192\n\t" \
    "ds_read_b128 a[176:179], v0 offset:12288\n\t" \
    "ds_read_b128 a[180:183], v1 offset:12288\n\t" \
    "ds_read_b128 a[184:187], v2 offset:12288\n\t" \
    "ds_read_b128 a[188:191], v3 offset:12288\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:0\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:0\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:0\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:0\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:4096\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:4096\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:4096\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:4096\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:22528\n\t" \
    "s_waitcnt lgkmcnt(15)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[128:131], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[128:131], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v160, v0, v1, v2\n\t" \
    "v_max3_f32 v160, v160, v3, v4\n\t" \
    "v_max3_f32 v160, v160, v5, v6\n\t" \
    "v_max3_f32 v160, v160, v7, v8\n\t" \
    "v_max3_f32 v160, v160, v9, v10\n\t" \
    "v_max3_f32 v160, v160, v11, v12\n\t" \
    "v_max3_f32 v160, v160, v13, v14\n\t" \
    "v_max3_f32 v160, v160, v15, v16\n\t" \
    "v_max3_f32 v160, v160, v17, v18\n\t" \
    "v_max3_f32 v160, v160, v19, v20\n\t" \
    "v_max3_f32 v160, v160, v21, v22\n\t" \
    "v_max3_f32 v160, v160, v23, v24\n\t" \
    "v_max3_f32 v160, v160, v25, v26\n\t" \
    "v_max3_f32 v160, v160, v27, v28\n\t" \
    "v_max3_f32 v160, v160, v29, v30\n\t" \
    "v_max_f32 v160, v160, v31\n\t" \
    "v_mov_b32 v188, v160\n\t" \
    "v_mov_b32 v189, v160\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v160, v188, v189\n\t" \
    "v_sub_f32 v64, 0, v160\n\t" \
    "v_mov_b32 v65, v64\n\t" \
    "v_mov_b32 v66, v64\n\t" \
    "v_mov_b32 v67, v64\n\t" \
    "v_mov_b32 v68, v64\n\t" \
    "v_mov_b32 v69, v64\n\t" \
    "v_mov_b32 v70, v64\n\t" \
    "v_mov_b32 v71, v64\n\t" \
    "v_mov_b32 v72, v64\n\t" \
    "v_mov_b32 v73, v64\n\t" \
    "v_mov_b32 v74, v64\n\t" \
    "v_mov_b32 v75, v64\n\t" \
    "v_mov_b32 v76, v64\n\t" \
    "v_mov_b32 v77, v64\n\t" \
    "v_mov_b32 v78, v64\n\t" \
    "v_mov_b32 v79, v64\n\t" \
    "v_sub_f32 v0, v0, v160\n\t" \
    "v_sub_f32 v1, v1, v160\n\t" \
    "v_sub_f32 v2, v2, v160\n\t" \
    "v_sub_f32 v3, v3, v160\n\t" \
    "v_sub_f32 v4, v4, v160\n\t" \
    "v_sub_f32 v5, v5, v160\n\t" \
    "v_sub_f32 v6, v6, v160\n\t" \
    "v_sub_f32 v7, v7, v160\n\t" \
    "v_sub_f32 v8, v8, v160\n\t" \
    "v_sub_f32 v9, v9, v160\n\t" \
    "v_sub_f32 v10, v10, v160\n\t" \
    "v_sub_f32 v11, v11, v160\n\t" \
    "v_sub_f32 v12, v12, v160\n\t" \
    "v_sub_f32 v13, v13, v160\n\t" \
    "v_sub_f32 v14, v14, v160\n\t" \
    "v_sub_f32 v15, v15, v160\n\t" \
    "v_sub_f32 v16, v16, v160\n\t" \
    "v_sub_f32 v17, v17, v160\n\t" \
    "v_sub_f32 v18, v18, v160\n\t" \
    "v_sub_f32 v19, v19, v160\n\t" \
    "v_sub_f32 v20, v20, v160\n\t" \
    "v_sub_f32 v21, v21, v160\n\t" \
    "v_sub_f32 v22, v22, v160\n\t" \
    "v_sub_f32 v23, v23, v160\n\t" \
    "v_sub_f32 v24, v24, v160\n\t" \
    "v_sub_f32 v25, v25, v160\n\t" \
    "v_sub_f32 v26, v26, v160\n\t" \
    "v_sub_f32 v27, v27, v160\n\t" \
    "v_sub_f32 v28, v28, v160\n\t" \
    "v_sub_f32 v29, v29, v160\n\t" \
    "v_sub_f32 v30, v30, v160\n\t" \
    "v_sub_f32 v31, v31, v160\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v168, v0, v4\n\t" \
    "v_add_f32 v169, v1, v5\n\t" \
    "v_add_f32 v170, v2, v6\n\t" \
    "v_add_f32 v171, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v168, v168, v8\n\t" \
    "v_add_f32 v168, v168, v12\n\t" \
    "v_add_f32 v169, v169, v9\n\t" \
    "v_add_f32 v169, v169, v13\n\t" \
    "v_add_f32 v170, v170, v10\n\t" \
    "v_add_f32 v170, v170, v14\n\t" \
    "v_add_f32 v171, v171, v11\n\t" \
    "v_add_f32 v171, v171, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v168, v168, v16\n\t" \
    "v_add_f32 v168, v168, v20\n\t" \
    "v_add_f32 v169, v169, v17\n\t" \
    "v_add_f32 v169, v169, v21\n\t" \
    "v_add_f32 v170, v170, v18\n\t" \
    "v_add_f32 v170, v170, v22\n\t" \
    "v_add_f32 v171, v171, v19\n\t" \
    "v_add_f32 v171, v171, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v168, v168, v24\n\t" \
    "v_add_f32 v168, v168, v28\n\t" \
    "v_add_f32 v169, v169, v25\n\t" \
    "v_add_f32 v169, v169, v29\n\t" \
    "v_add_f32 v170, v170, v26\n\t" \
    "v_add_f32 v170, v170, v30\n\t" \
    "v_add_f32 v171, v171, v27\n\t" \
    "v_add_f32 v171, v171, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v184, v168, v170\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(14)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(12)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(10)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(8)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], 0\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[144:147], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[144:147], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v161, v32, v33, v34\n\t" \
    "v_max3_f32 v161, v161, v35, v36\n\t" \
    "v_max3_f32 v161, v161, v37, v38\n\t" \
    "v_max3_f32 v161, v161, v39, v40\n\t" \
    "v_max3_f32 v161, v161, v41, v42\n\t" \
    "v_max3_f32 v161, v161, v43, v44\n\t" \
    "v_max3_f32 v161, v161, v45, v46\n\t" \
    "v_max3_f32 v161, v161, v47, v48\n\t" \
    "v_max3_f32 v161, v161, v49, v50\n\t" \
    "v_max3_f32 v161, v161, v51, v52\n\t" \
    "v_max3_f32 v161, v161, v53, v54\n\t" \
    "v_max3_f32 v161, v161, v55, v56\n\t" \
    "v_max3_f32 v161, v161, v57, v58\n\t" \
    "v_max3_f32 v161, v161, v59, v60\n\t" \
    "v_max3_f32 v161, v161, v61, v62\n\t" \
    "v_max_f32 v161, v161, v63\n\t" \
    "v_mov_b32 v188, v161\n\t" \
    "v_mov_b32 v189, v161\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v161, v188, v189\n\t" \
    "v_sub_f32 v80, 0, v161\n\t" \
    "v_mov_b32 v81, v80\n\t" \
    "v_mov_b32 v82, v80\n\t" \
    "v_mov_b32 v83, v80\n\t" \
    "v_mov_b32 v84, v80\n\t" \
    "v_mov_b32 v85, v80\n\t" \
    "v_mov_b32 v86, v80\n\t" \
    "v_mov_b32 v87, v80\n\t" \
    "v_mov_b32 v88, v80\n\t" \
    "v_mov_b32 v89, v80\n\t" \
    "v_mov_b32 v90, v80\n\t" \
    "v_mov_b32 v91, v80\n\t" \
    "v_mov_b32 v92, v80\n\t" \
    "v_mov_b32 v93, v80\n\t" \
    "v_mov_b32 v94, v80\n\t" \
    "v_mov_b32 v95, v80\n\t" \
    "v_sub_f32 v32, v32, v161\n\t" \
    "v_sub_f32 v33, v33, v161\n\t" \
    "v_sub_f32 v34, v34, v161\n\t" \
    "v_sub_f32 v35, v35, v161\n\t" \
    "v_sub_f32 v36, v36, v161\n\t" \
    "v_sub_f32 v37, v37, v161\n\t" \
    "v_sub_f32 v38, v38, v161\n\t" \
    "v_sub_f32 v39, v39, v161\n\t" \
    "v_sub_f32 v40, v40, v161\n\t" \
    "v_sub_f32 v41, v41, v161\n\t" \
    "v_sub_f32 v42, v42, v161\n\t" \
    "v_sub_f32 v43, v43, v161\n\t" \
    "v_sub_f32 v44, v44, v161\n\t" \
    "v_sub_f32 v45, v45, v161\n\t" \
    "v_sub_f32 v46, v46, v161\n\t" \
    "v_sub_f32 v47, v47, v161\n\t" \
    "v_sub_f32 v48, v48, v161\n\t" \
    "v_sub_f32 v49, v49, v161\n\t" \
    "v_sub_f32 v50, v50, v161\n\t" \
    "v_sub_f32 v51, v51, v161\n\t" \
    "v_sub_f32 v52, v52, v161\n\t" \
    "v_sub_f32 v53, v53, v161\n\t" \
    "v_sub_f32 v54, v54, v161\n\t" \
    "v_sub_f32 v55, v55, v161\n\t" \
    "v_sub_f32 v56, v56, v161\n\t" \
    "v_sub_f32 v57, v57, v161\n\t" \
    "v_sub_f32 v58, v58, v161\n\t" \
    "v_sub_f32 v59, v59, v161\n\t" \
    "v_sub_f32 v60, v60, v161\n\t" \
    "v_sub_f32 v61, v61, v161\n\t" \
    "v_sub_f32 v62, v62, v161\n\t" \
    "v_sub_f32 v63, v63, v161\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v172, v32, v36\n\t" \
    "v_add_f32 v173, v33, v37\n\t" \
    "v_add_f32 v174, v34, v38\n\t" \
    "v_add_f32 v175, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v172, v172, v40\n\t" \
    "v_add_f32 v172, v172, v44\n\t" \
    "v_add_f32 v173, v173, v41\n\t" \
    "v_add_f32 v173, v173, v45\n\t" \
    "v_add_f32 v174, v174, v42\n\t" \
    "v_add_f32 v174, v174, v46\n\t" \
    "v_add_f32 v175, v175, v43\n\t" \
    "v_add_f32 v175, v175, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v172, v172, v48\n\t" \
    "v_add_f32 v172, v172, v52\n\t" \
    "v_add_f32 v173, v173, v49\n\t" \
    "v_add_f32 v173, v173, v53\n\t" \
    "v_add_f32 v174, v174, v50\n\t" \
    "v_add_f32 v174, v174, v54\n\t" \
    "v_add_f32 v175, v175, v51\n\t" \
    "v_add_f32 v175, v175, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v172, v172, v56\n\t" \
    "v_add_f32 v172, v172, v60\n\t" \
    "v_add_f32 v173, v173, v57\n\t" \
    "v_add_f32 v173, v173, v61\n\t" \
    "v_add_f32 v174, v174, v58\n\t" \
    "v_add_f32 v174, v174, v62\n\t" \
    "v_add_f32 v175, v175, v59\n\t" \
    "v_add_f32 v175, v175, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v172, v172, v173\n\t" \
    "v_add_f32 v174, v174, v175\n\t" \
    "v_add_f32 v185, v172, v174\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[192:195], v[32:35], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[208:211], v[32:35], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[160:163], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v162, v0, v1, v2\n\t" \
    "v_max3_f32 v162, v162, v3, v4\n\t" \
    "v_max3_f32 v162, v162, v5, v6\n\t" \
    "v_max3_f32 v162, v162, v7, v8\n\t" \
    "v_max3_f32 v162, v162, v9, v10\n\t" \
    "v_max3_f32 v162, v162, v11, v12\n\t" \
    "v_max3_f32 v162, v162, v13, v14\n\t" \
    "v_max3_f32 v162, v162, v15, v16\n\t" \
    "v_max3_f32 v162, v162, v17, v18\n\t" \
    "v_max3_f32 v162, v162, v19, v20\n\t" \
    "v_max3_f32 v162, v162, v21, v22\n\t" \
    "v_max3_f32 v162, v162, v23, v24\n\t" \
    "v_max3_f32 v162, v162, v25, v26\n\t" \
    "v_max3_f32 v162, v162, v27, v28\n\t" \
    "v_max3_f32 v162, v162, v29, v30\n\t" \
    "v_max_f32 v162, v162, v31\n\t" \
    "v_mov_b32 v188, v162\n\t" \
    "v_mov_b32 v189, v162\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v162, v188, v189\n\t" \
    "v_sub_f32 v96, 0, v162\n\t" \
    "v_mov_b32 v97, v96\n\t" \
    "v_mov_b32 v98, v96\n\t" \
    "v_mov_b32 v99, v96\n\t" \
    "v_mov_b32 v100, v96\n\t" \
    "v_mov_b32 v101, v96\n\t" \
    "v_mov_b32 v102, v96\n\t" \
    "v_mov_b32 v103, v96\n\t" \
    "v_mov_b32 v104, v96\n\t" \
    "v_mov_b32 v105, v96\n\t" \
    "v_mov_b32 v106, v96\n\t" \
    "v_mov_b32 v107, v96\n\t" \
    "v_mov_b32 v108, v96\n\t" \
    "v_mov_b32 v109, v96\n\t" \
    "v_mov_b32 v110, v96\n\t" \
    "v_mov_b32 v111, v96\n\t" \
    "v_sub_f32 v0, v0, v162\n\t" \
    "v_sub_f32 v1, v1, v162\n\t" \
    "v_sub_f32 v2, v2, v162\n\t" \
    "v_sub_f32 v3, v3, v162\n\t" \
    "v_sub_f32 v4, v4, v162\n\t" \
    "v_sub_f32 v5, v5, v162\n\t" \
    "v_sub_f32 v6, v6, v162\n\t" \
    "v_sub_f32 v7, v7, v162\n\t" \
    "v_sub_f32 v8, v8, v162\n\t" \
    "v_sub_f32 v9, v9, v162\n\t" \
    "v_sub_f32 v10, v10, v162\n\t" \
    "v_sub_f32 v11, v11, v162\n\t" \
    "v_sub_f32 v12, v12, v162\n\t" \
    "v_sub_f32 v13, v13, v162\n\t" \
    "v_sub_f32 v14, v14, v162\n\t" \
    "v_sub_f32 v15, v15, v162\n\t" \
    "v_sub_f32 v16, v16, v162\n\t" \
    "v_sub_f32 v17, v17, v162\n\t" \
    "v_sub_f32 v18, v18, v162\n\t" \
    "v_sub_f32 v19, v19, v162\n\t" \
    "v_sub_f32 v20, v20, v162\n\t" \
    "v_sub_f32 v21, v21, v162\n\t" \
    "v_sub_f32 v22, v22, v162\n\t" \
    "v_sub_f32 v23, v23, v162\n\t" \
    "v_sub_f32 v24, v24, v162\n\t" \
    "v_sub_f32 v25, v25, v162\n\t" \
    "v_sub_f32 v26, v26, v162\n\t" \
    "v_sub_f32 v27, v27, v162\n\t" \
    "v_sub_f32 v28, v28, v162\n\t" \
    "v_sub_f32 v29, v29, v162\n\t" \
    "v_sub_f32 v30, v30, v162\n\t" \
    "v_sub_f32 v31, v31, v162\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v176, v0, v4\n\t" \
    "v_add_f32 v177, v1, v5\n\t" \
    "v_add_f32 v178, v2, v6\n\t" \
    "v_add_f32 v179, v3, v7\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v176, v176, v8\n\t" \
    "v_add_f32 v176, v176, v12\n\t" \
    "v_add_f32 v177, v177, v9\n\t" \
    "v_add_f32 v177, v177, v13\n\t" \
    "v_add_f32 v178, v178, v10\n\t" \
    "v_add_f32 v178, v178, v14\n\t" \
    "v_add_f32 v179, v179, v11\n\t" \
    "v_add_f32 v179, v179, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v176, v176, v16\n\t" \
    "v_add_f32 v176, v176, v20\n\t" \
    "v_add_f32 v177, v177, v17\n\t" \
    "v_add_f32 v177, v177, v21\n\t" \
    "v_add_f32 v178, v178, v18\n\t" \
    "v_add_f32 v178, v178, v22\n\t" \
    "v_add_f32 v179, v179, v19\n\t" \
    "v_add_f32 v179, v179, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v176, v176, v24\n\t" \
    "v_add_f32 v176, v176, v28\n\t" \
    "v_add_f32 v177, v177, v25\n\t" \
    "v_add_f32 v177, v177, v29\n\t" \
    "v_add_f32 v178, v178, v26\n\t" \
    "v_add_f32 v178, v178, v30\n\t" \
    "v_add_f32 v179, v179, v27\n\t" \
    "v_add_f32 v179, v179, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v176, v176, v177\n\t" \
    "v_add_f32 v178, v178, v179\n\t" \
    "v_add_f32 v186, v176, v178\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[0:3], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[176:179], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[176:179], 0\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "s_nop 7\n\t" \
    "v_max3_f32 v163, v32, v33, v34\n\t" \
    "v_max3_f32 v163, v163, v35, v36\n\t" \
    "v_max3_f32 v163, v163, v37, v38\n\t" \
    "v_max3_f32 v163, v163, v39, v40\n\t" \
    "v_max3_f32 v163, v163, v41, v42\n\t" \
    "v_max3_f32 v163, v163, v43, v44\n\t" \
    "v_max3_f32 v163, v163, v45, v46\n\t" \
    "v_max3_f32 v163, v163, v47, v48\n\t" \
    "v_max3_f32 v163, v163, v49, v50\n\t" \
    "v_max3_f32 v163, v163, v51, v52\n\t" \
    "v_max3_f32 v163, v163, v53, v54\n\t" \
    "v_max3_f32 v163, v163, v55, v56\n\t" \
    "v_max3_f32 v163, v163, v57, v58\n\t" \
    "v_max3_f32 v163, v163, v59, v60\n\t" \
    "v_max3_f32 v163, v163, v61, v62\n\t" \
    "v_max_f32 v163, v163, v63\n\t" \
    "v_mov_b32 v188, v163\n\t" \
    "v_mov_b32 v189, v163\n\t" \
    "s_nop 1\n\t" \
    "v_permlane32_swap_b32 v188, v189\n\t" \
    "s_nop 1\n\t" \
    "v_max_f32 v163, v188, v189\n\t" \
    "v_sub_f32 v112, 0, v163\n\t" \
    "v_mov_b32 v113, v112\n\t" \
    "v_mov_b32 v114, v112\n\t" \
    "v_mov_b32 v115, v112\n\t" \
    "v_mov_b32 v116, v112\n\t" \
    "v_mov_b32 v117, v112\n\t" \
    "v_mov_b32 v118, v112\n\t" \
    "v_mov_b32 v119, v112\n\t" \
    "v_mov_b32 v120, v112\n\t" \
    "v_mov_b32 v121, v112\n\t" \
    "v_mov_b32 v122, v112\n\t" \
    "v_mov_b32 v123, v112\n\t" \
    "v_mov_b32 v124, v112\n\t" \
    "v_mov_b32 v125, v112\n\t" \
    "v_mov_b32 v126, v112\n\t" \
    "v_mov_b32 v127, v112\n\t" \
    "v_sub_f32 v32, v32, v163\n\t" \
    "v_sub_f32 v33, v33, v163\n\t" \
    "v_sub_f32 v34, v34, v163\n\t" \
    "v_sub_f32 v35, v35, v163\n\t" \
    "v_sub_f32 v36, v36, v163\n\t" \
    "v_sub_f32 v37, v37, v163\n\t" \
    "v_sub_f32 v38, v38, v163\n\t" \
    "v_sub_f32 v39, v39, v163\n\t" \
    "v_sub_f32 v40, v40, v163\n\t" \
    "v_sub_f32 v41, v41, v163\n\t" \
    "v_sub_f32 v42, v42, v163\n\t" \
    "v_sub_f32 v43, v43, v163\n\t" \
    "v_sub_f32 v44, v44, v163\n\t" \
    "v_sub_f32 v45, v45, v163\n\t" \
    "v_sub_f32 v46, v46, v163\n\t" \
    "v_sub_f32 v47, v47, v163\n\t" \
    "v_sub_f32 v48, v48, v163\n\t" \
    "v_sub_f32 v49, v49, v163\n\t" \
    "v_sub_f32 v50, v50, v163\n\t" \
    "v_sub_f32 v51, v51, v163\n\t" \
    "v_sub_f32 v52, v52, v163\n\t" \
    "v_sub_f32 v53, v53, v163\n\t" \
    "v_sub_f32 v54, v54, v163\n\t" \
    "v_sub_f32 v55, v55, v163\n\t" \
    "v_sub_f32 v56, v56, v163\n\t" \
    "v_sub_f32 v57, v57, v163\n\t" \
    "v_sub_f32 v58, v58, v163\n\t" \
    "v_sub_f32 v59, v59, v163\n\t" \
    "v_sub_f32 v60, v60, v163\n\t" \
    "v_sub_f32 v61, v61, v163\n\t" \
    "v_sub_f32 v62, v62, v163\n\t" \
    "v_sub_f32 v63, v63, v163\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v180, v32, v36\n\t" \
    "v_add_f32 v181, v33, v37\n\t" \
    "v_add_f32 v182, v34, v38\n\t" \
    "v_add_f32 v183, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v180, v180, v40\n\t" \
    "v_add_f32 v180, v180, v44\n\t" \
    "v_add_f32 v181, v181, v41\n\t" \
    "v_add_f32 v181, v181, v45\n\t" \
    "v_add_f32 v182, v182, v42\n\t" \
    "v_add_f32 v182, v182, v46\n\t" \
    "v_add_f32 v183, v183, v43\n\t" \
    "v_add_f32 v183, v183, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_accvgpr_write_b32 a96, 0\n\t" \
    "v_accvgpr_write_b32 a97, 0\n\t" \
    "v_accvgpr_write_b32 a98, 0\n\t" \
    "v_accvgpr_write_b32 a99, 0\n\t" \
    "v_accvgpr_write_b32 a100, 0\n\t" \
    "v_accvgpr_write_b32 a101, 0\n\t" \
    "v_accvgpr_write_b32 a102, 0\n\t" \
    "v_accvgpr_write_b32 a103, 0\n\t" \
    "v_accvgpr_write_b32 a104, 0\n\t" \
    "v_accvgpr_write_b32 a105, 0\n\t" \
    "v_accvgpr_write_b32 a106, 0\n\t" \
    "v_accvgpr_write_b32 a107, 0\n\t" \
    "v_accvgpr_write_b32 a108, 0\n\t" \
    "v_accvgpr_write_b32 a109, 0\n\t" \
    "v_accvgpr_write_b32 a110, 0\n\t" \
    "v_accvgpr_write_b32 a111, 0\n\t" \
    "v_accvgpr_write_b32 a112, 0\n\t" \
    "v_accvgpr_write_b32 a113, 0\n\t" \
    "v_accvgpr_write_b32 a114, 0\n\t" \
    "v_accvgpr_write_b32 a115, 0\n\t" \
    "v_accvgpr_write_b32 a116, 0\n\t" \
    "v_accvgpr_write_b32 a117, 0\n\t" \
    "v_accvgpr_write_b32 a118, 0\n\t" \
    "v_accvgpr_write_b32 a119, 0\n\t" \
    "v_accvgpr_write_b32 a120, 0\n\t" \
    "v_accvgpr_write_b32 a121, 0\n\t" \
    "v_accvgpr_write_b32 a122, 0\n\t" \
    "v_accvgpr_write_b32 a123, 0\n\t" \
    "v_accvgpr_write_b32 a124, 0\n\t" \
    "v_accvgpr_write_b32 a125, 0\n\t" \
    "v_accvgpr_write_b32 a126, 0\n\t" \
    "v_accvgpr_write_b32 a127, 0\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:8192\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:8192\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:8192\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:8192\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:12288\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:12288\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:12288\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:12288\n\t" \
    "FA2HS_LOOP_%=:\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:0\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v180, v180, v48\n\t" \
    "v_add_f32 v180, v180, v52\n\t" \
    "v_add_f32 v181, v181, v49\n\t" \
    "v_add_f32 v181, v181, v53\n\t" \
    "v_add_f32 v182, v182, v50\n\t" \
    "v_add_f32 v182, v182, v54\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_add_f32 v183, v183, v51\n\t" \
    "v_add_f32 v183, v183, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[128:131], v[64:79]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:4096\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v180, v180, v56\n\t" \
    "v_add_f32 v180, v180, v60\n\t" \
    "v_add_f32 v181, v181, v57\n\t" \
    "v_add_f32 v181, v181, v61\n\t" \
    "v_add_f32 v182, v182, v58\n\t" \
    "v_add_f32 v182, v182, v62\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "v_add_f32 v183, v183, v59\n\t" \
    "v_add_f32 v183, v183, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v180, v180, v181\n\t" \
    "v_add_f32 v182, v182, v183\n\t" \
    "v_add_f32 v187, v180, v182\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:16384\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v168, v0, v4\n\t" \
    "v_add_f32 v169, v1, v5\n\t" \
    "v_add_f32 v170, v2, v6\n\t" \
    "v_add_f32 v171, v3, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v168, v168, v8\n\t" \
    "v_add_f32 v168, v168, v12\n\t" \
    "v_add_f32 v169, v169, v9\n\t" \
    "v_add_f32 v169, v169, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "v_add_f32 v170, v170, v10\n\t" \
    "v_add_f32 v170, v170, v14\n\t" \
    "v_add_f32 v171, v171, v11\n\t" \
    "v_add_f32 v171, v171, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:24576\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:24576\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:26624\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:26624\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:28672\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:30720\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:30720\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v168, v168, v16\n\t" \
    "v_add_f32 v168, v168, v20\n\t" \
    "v_add_f32 v169, v169, v17\n\t" \
    "v_add_f32 v169, v169, v21\n\t" \
    "v_add_f32 v170, v170, v18\n\t" \
    "v_add_f32 v170, v170, v22\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_add_f32 v171, v171, v19\n\t" \
    "v_add_f32 v171, v171, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v168, v168, v24\n\t" \
    "v_add_f32 v168, v168, v28\n\t" \
    "v_add_f32 v169, v169, v25\n\t" \
    "v_add_f32 v169, v169, v29\n\t" \
    "v_add_f32 v170, v170, v26\n\t" \
    "v_add_f32 v170, v170, v30\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "v_add_f32 v171, v171, v27\n\t" \
    "v_add_f32 v171, v171, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v184, v168, v170\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v172, v32, v36\n\t" \
    "v_add_f32 v173, v33, v37\n\t" \
    "v_add_f32 v174, v34, v38\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_add_f32 v175, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v172, v172, v40\n\t" \
    "v_add_f32 v172, v172, v44\n\t" \
    "v_add_f32 v173, v173, v41\n\t" \
    "v_add_f32 v173, v173, v45\n\t" \
    "v_add_f32 v174, v174, v42\n\t" \
    "v_add_f32 v174, v174, v46\n\t" \
    "v_add_f32 v175, v175, v43\n\t" \
    "v_add_f32 v175, v175, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v172, v172, v48\n\t" \
    "v_add_f32 v172, v172, v52\n\t" \
    "v_add_f32 v173, v173, v49\n\t" \
    "v_add_f32 v173, v173, v53\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_add_f32 v174, v174, v50\n\t" \
    "v_add_f32 v174, v174, v54\n\t" \
    "v_add_f32 v175, v175, v51\n\t" \
    "v_add_f32 v175, v175, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v172, v172, v56\n\t" \
    "v_add_f32 v172, v172, v60\n\t" \
    "v_add_f32 v173, v173, v57\n\t" \
    "v_add_f32 v173, v173, v61\n\t" \
    "v_add_f32 v174, v174, v58\n\t" \
    "v_add_f32 v174, v174, v62\n\t" \
    "v_add_f32 v175, v175, v59\n\t" \
    "v_add_f32 v175, v175, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v172, v172, v173\n\t" \
    "v_add_f32 v174, v174, v175\n\t" \
    "v_add_f32 v185, v172, v174\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[192:195], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v176, v0, v4\n\t" \
    "v_add_f32 v177, v1, v5\n\t" \
    "v_add_f32 v178, v2, v6\n\t" \
    "v_add_f32 v179, v3, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[208:211], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v176, v176, v8\n\t" \
    "v_add_f32 v176, v176, v12\n\t" \
    "v_add_f32 v177, v177, v9\n\t" \
    "v_add_f32 v177, v177, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_add_f32 v178, v178, v10\n\t" \
    "v_add_f32 v178, v178, v14\n\t" \
    "v_add_f32 v179, v179, v11\n\t" \
    "v_add_f32 v179, v179, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v176, v176, v16\n\t" \
    "v_add_f32 v176, v176, v20\n\t" \
    "v_add_f32 v177, v177, v17\n\t" \
    "v_add_f32 v177, v177, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_add_f32 v178, v178, v18\n\t" \
    "v_add_f32 v178, v178, v22\n\t" \
    "v_add_f32 v179, v179, v19\n\t" \
    "v_add_f32 v179, v179, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v176, v176, v24\n\t" \
    "v_add_f32 v176, v176, v28\n\t" \
    "v_add_f32 v177, v177, v25\n\t" \
    "v_add_f32 v177, v177, v29\n\t" \
    "v_add_f32 v178, v178, v26\n\t" \
    "v_add_f32 v178, v178, v30\n\t" \
    "v_add_f32 v179, v179, v27\n\t" \
    "v_add_f32 v179, v179, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v176, v176, v177\n\t" \
    "v_add_f32 v178, v178, v179\n\t" \
    "v_add_f32 v186, v176, v178\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:0\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:0\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:0\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:0\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[0:3], a[64:79]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:4096\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:4096\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:4096\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:4096\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v180, v32, v36\n\t" \
    "v_add_f32 v181, v33, v37\n\t" \
    "v_add_f32 v182, v34, v38\n\t" \
    "v_add_f32 v183, v35, v39\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[0:3], a[80:95]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v180, v180, v40\n\t" \
    "v_add_f32 v180, v180, v44\n\t" \
    "v_add_f32 v181, v181, v41\n\t" \
    "v_add_f32 v181, v181, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_add_f32 v182, v182, v42\n\t" \
    "v_add_f32 v182, v182, v46\n\t" \
    "v_add_f32 v183, v183, v43\n\t" \
    "v_add_f32 v183, v183, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_eq_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_EPI_%=\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "s_waitcnt lgkmcnt(7)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[128:131], v[64:79]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[132:135], v[0:15]\n\t" \
    "s_waitcnt vmcnt(7)\n\t" \
    "v_cvt_pk_bf16_f32 v128, v128, v129\n\t" \
    "v_cvt_pk_bf16_f32 v129, v130, v131\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "s_waitcnt vmcnt(6)\n\t" \
    "v_cvt_pk_bf16_f32 v130, v132, v133\n\t" \
    "v_cvt_pk_bf16_f32 v131, v134, v135\n\t" \
    "ds_write_b128 %[lo], v[128:131] offset:8192\n\t" \
    "s_waitcnt lgkmcnt(6)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[136:139], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v180, v180, v48\n\t" \
    "v_add_f32 v180, v180, v52\n\t" \
    "v_add_f32 v181, v181, v49\n\t" \
    "v_add_f32 v181, v181, v53\n\t" \
    "v_add_f32 v182, v182, v50\n\t" \
    "v_add_f32 v182, v182, v54\n\t" \
    "s_waitcnt lgkmcnt(5)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[140:143], v[0:15]\n\t" \
    "v_add_f32 v183, v183, v51\n\t" \
    "v_add_f32 v183, v183, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[128:131], v[64:79]\n\t" \
    "s_waitcnt vmcnt(5)\n\t" \
    "v_cvt_pk_bf16_f32 v136, v136, v137\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_cvt_pk_bf16_f32 v137, v138, v139\n\t" \
    "s_waitcnt vmcnt(4)\n\t" \
    "v_cvt_pk_bf16_f32 v138, v140, v141\n\t" \
    "v_cvt_pk_bf16_f32 v139, v142, v143\n\t" \
    "ds_write_b128 %[lo], v[136:139] offset:12288\n\t" \
    "s_waitcnt lgkmcnt(4)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[132:135], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "s_waitcnt lgkmcnt(3)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[136:139], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v180, v180, v56\n\t" \
    "v_add_f32 v180, v180, v60\n\t" \
    "v_add_f32 v181, v181, v57\n\t" \
    "v_add_f32 v181, v181, v61\n\t" \
    "v_add_f32 v182, v182, v58\n\t" \
    "v_add_f32 v182, v182, v62\n\t" \
    "s_waitcnt lgkmcnt(2)\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[140:143], v[16:31]\n\t" \
    "v_add_f32 v183, v183, v59\n\t" \
    "v_add_f32 v183, v183, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v180, v180, v181\n\t" \
    "v_add_f32 v182, v182, v183\n\t" \
    "v_add_f32 v187, v180, v182\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "s_waitcnt vmcnt(3)\n\t" \
    "v_cvt_pk_bf16_f32 v144, v144, v145\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "v_cvt_pk_bf16_f32 v145, v146, v147\n\t" \
    "s_waitcnt vmcnt(2)\n\t" \
    "v_cvt_pk_bf16_f32 v146, v148, v149\n\t" \
    "v_cvt_pk_bf16_f32 v147, v150, v151\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "ds_write_b128 %[lo], v[144:147] offset:24576\n\t" \
    "s_waitcnt vmcnt(1)\n\t" \
    "v_cvt_pk_bf16_f32 v152, v152, v153\n\t" \
    "v_cvt_pk_bf16_f32 v153, v154, v155\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "s_waitcnt vmcnt(0)\n\t" \
    "v_cvt_pk_bf16_f32 v154, v156, v157\n\t" \
    "v_cvt_pk_bf16_f32 v155, v158, v159\n\t" \
    "ds_write_b128 %[lo], v[152:155] offset:28672\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v168, v0, v4\n\t" \
    "v_add_f32 v169, v1, v5\n\t" \
    "v_add_f32 v170, v2, v6\n\t" \
    "v_add_f32 v171, v3, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v168, v168, v8\n\t" \
    "v_add_f32 v168, v168, v12\n\t" \
    "v_add_f32 v169, v169, v9\n\t" \
    "v_add_f32 v169, v169, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "v_add_f32 v170, v170, v10\n\t" \
    "v_add_f32 v170, v170, v14\n\t" \
    "v_add_f32 v171, v171, v11\n\t" \
    "v_add_f32 v171, v171, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "ds_read_b64_tr_b16 a[192:193], %[va0_0] offset:16384\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "ds_read_b64_tr_b16 a[194:195], %[va0_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[196:197], %[va0_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[198:199], %[va0_1] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[200:201], %[va0_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[202:203], %[va0_1] offset:20480\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "ds_read_b64_tr_b16 a[204:205], %[va0_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[206:207], %[va0_1] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[208:209], %[va1_0] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[210:211], %[va1_1] offset:16384\n\t" \
    "ds_read_b64_tr_b16 a[212:213], %[va1_0] offset:18432\n\t" \
    "ds_read_b64_tr_b16 a[214:215], %[va1_1] offset:18432\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[148:151], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "ds_read_b64_tr_b16 a[216:217], %[va1_0] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[218:219], %[va1_1] offset:20480\n\t" \
    "ds_read_b64_tr_b16 a[220:221], %[va1_0] offset:22528\n\t" \
    "ds_read_b64_tr_b16 a[222:223], %[va1_1] offset:22528\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[152:155], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v168, v168, v16\n\t" \
    "v_add_f32 v168, v168, v20\n\t" \
    "v_add_f32 v169, v169, v17\n\t" \
    "v_add_f32 v169, v169, v21\n\t" \
    "v_add_f32 v170, v170, v18\n\t" \
    "v_add_f32 v170, v170, v22\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[156:159], v[32:47]\n\t" \
    "v_add_f32 v171, v171, v19\n\t" \
    "v_add_f32 v171, v171, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[144:147], v[80:95]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[148:151], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[152:155], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v168, v168, v24\n\t" \
    "v_add_f32 v168, v168, v28\n\t" \
    "v_add_f32 v169, v169, v25\n\t" \
    "v_add_f32 v169, v169, v29\n\t" \
    "v_add_f32 v170, v170, v26\n\t" \
    "v_add_f32 v170, v170, v30\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[156:159], v[48:63]\n\t" \
    "v_add_f32 v171, v171, v27\n\t" \
    "v_add_f32 v171, v171, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v168, v168, v169\n\t" \
    "v_add_f32 v170, v170, v171\n\t" \
    "v_add_f32 v184, v168, v170\n\t" \
    "v_add_f32 v164, v164, v184\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v184\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    "s_barrier\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "buffer_load_dwordx4 v[128:131], %[vo0], %[rsk], %[goff] offen\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "buffer_load_dwordx4 v[132:135], %[vo0], %[rsk], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[136:139], %[vo1], %[rsk], %[goff] offen\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[192:195], v[0:3], a[0:15]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "buffer_load_dwordx4 v[140:143], %[vo1], %[rsk], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[196:199], v[8:11], a[0:15]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[200:203], v[16:19], a[0:15]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v172, v32, v36\n\t" \
    "v_add_f32 v173, v33, v37\n\t" \
    "v_add_f32 v174, v34, v38\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[0:15], a[204:207], v[24:27], a[0:15]\n\t" \
    "v_add_f32 v175, v35, v39\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[208:211], v[0:3], a[16:31]\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[212:215], v[8:11], a[16:31]\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[216:219], v[16:19], a[16:31]\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[16:31], a[220:223], v[24:27], a[16:31]\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v172, v172, v40\n\t" \
    "v_add_f32 v172, v172, v44\n\t" \
    "v_add_f32 v173, v173, v41\n\t" \
    "v_add_f32 v173, v173, v45\n\t" \
    "v_add_f32 v174, v174, v42\n\t" \
    "v_add_f32 v174, v174, v46\n\t" \
    "v_add_f32 v175, v175, v43\n\t" \
    "v_add_f32 v175, v175, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[224:227], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[228:231], a[164:167], v[0:15]\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[232:235], a[168:171], v[0:15]\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v172, v172, v48\n\t" \
    "v_add_f32 v172, v172, v52\n\t" \
    "v_add_f32 v173, v173, v49\n\t" \
    "v_add_f32 v173, v173, v53\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[0:15], a[236:239], a[172:175], v[0:15]\n\t" \
    "v_add_f32 v174, v174, v50\n\t" \
    "v_add_f32 v174, v174, v54\n\t" \
    "v_add_f32 v175, v175, v51\n\t" \
    "v_add_f32 v175, v175, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[240:243], a[160:163], v[96:111]\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[244:247], a[164:167], v[16:31]\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[248:251], a[168:171], v[16:31]\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[16:31], a[252:255], a[172:175], v[16:31]\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v172, v172, v56\n\t" \
    "v_add_f32 v172, v172, v60\n\t" \
    "v_add_f32 v173, v173, v57\n\t" \
    "v_add_f32 v173, v173, v61\n\t" \
    "v_add_f32 v174, v174, v58\n\t" \
    "v_add_f32 v174, v174, v62\n\t" \
    "v_add_f32 v175, v175, v59\n\t" \
    "v_add_f32 v175, v175, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v172, v172, v173\n\t" \
    "v_add_f32 v174, v174, v175\n\t" \
    "v_add_f32 v185, v172, v174\n\t" \
    "v_add_f32 v165, v165, v185\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v185\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v0, v0\n\t" \
    "buffer_load_dwordx4 v[144:147], %[vo0], %[rsv], %[goff] offen\n\t" \
    "v_exp_f32 v1, v1\n\t" \
    "buffer_load_dwordx4 v[148:151], %[vo0], %[rsv], %[goff] offen offset:16\n\t" \
    "buffer_load_dwordx4 v[152:155], %[vo1], %[rsv], %[goff] offen\n\t" \
    "buffer_load_dwordx4 v[156:159], %[vo1], %[rsv], %[goff] offen offset:16\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[192:195], v[32:35], a[32:47]\n\t" \
    "v_exp_f32 v2, v2\n\t" \
    "v_exp_f32 v3, v3\n\t" \
    "s_add_u32 %[goff], %[goff], 16384\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[196:199], v[40:43], a[32:47]\n\t" \
    "v_exp_f32 v4, v4\n\t" \
    "v_exp_f32 v5, v5\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[200:203], v[48:51], a[32:47]\n\t" \
    "v_exp_f32 v6, v6\n\t" \
    "v_exp_f32 v7, v7\n\t" \
    "v_add_f32 v176, v0, v4\n\t" \
    "v_add_f32 v177, v1, v5\n\t" \
    "v_add_f32 v178, v2, v6\n\t" \
    "v_add_f32 v179, v3, v7\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[32:47], a[204:207], v[56:59], a[32:47]\n\t" \
    "v_cvt_pk_bf16_f32 v0, v0, v1\n\t" \
    "v_cvt_pk_bf16_f32 v1, v2, v3\n\t" \
    "v_cvt_pk_bf16_f32 v2, v4, v5\n\t" \
    "v_cvt_pk_bf16_f32 v3, v6, v7\n\t" \
    "v_exp_f32 v8, v8\n\t" \
    "v_exp_f32 v9, v9\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[208:211], v[32:35], a[48:63]\n\t" \
    "v_exp_f32 v10, v10\n\t" \
    "v_exp_f32 v11, v11\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[212:215], v[40:43], a[48:63]\n\t" \
    "v_exp_f32 v12, v12\n\t" \
    "v_exp_f32 v13, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[216:219], v[48:51], a[48:63]\n\t" \
    "v_exp_f32 v14, v14\n\t" \
    "v_exp_f32 v15, v15\n\t" \
    "v_add_f32 v176, v176, v8\n\t" \
    "v_add_f32 v176, v176, v12\n\t" \
    "v_add_f32 v177, v177, v9\n\t" \
    "v_add_f32 v177, v177, v13\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[48:63], a[220:223], v[56:59], a[48:63]\n\t" \
    "v_add_f32 v178, v178, v10\n\t" \
    "v_add_f32 v178, v178, v14\n\t" \
    "v_add_f32 v179, v179, v11\n\t" \
    "v_add_f32 v179, v179, v15\n\t" \
    "v_cvt_pk_bf16_f32 v8, v8, v9\n\t" \
    "v_cvt_pk_bf16_f32 v9, v10, v11\n\t" \
    "v_cvt_pk_bf16_f32 v10, v12, v13\n\t" \
    "v_cvt_pk_bf16_f32 v11, v14, v15\n\t" \
    "v_exp_f32 v16, v16\n\t" \
    "v_exp_f32 v17, v17\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[224:227], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v18, v18\n\t" \
    "v_exp_f32 v19, v19\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[228:231], a[180:183], v[32:47]\n\t" \
    "v_exp_f32 v20, v20\n\t" \
    "v_exp_f32 v21, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[232:235], a[184:187], v[32:47]\n\t" \
    "v_exp_f32 v22, v22\n\t" \
    "v_exp_f32 v23, v23\n\t" \
    "v_add_f32 v176, v176, v16\n\t" \
    "v_add_f32 v176, v176, v20\n\t" \
    "v_add_f32 v177, v177, v17\n\t" \
    "v_add_f32 v177, v177, v21\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[32:47], a[236:239], a[188:191], v[32:47]\n\t" \
    "v_add_f32 v178, v178, v18\n\t" \
    "v_add_f32 v178, v178, v22\n\t" \
    "v_add_f32 v179, v179, v19\n\t" \
    "v_add_f32 v179, v179, v23\n\t" \
    "v_cvt_pk_bf16_f32 v16, v16, v17\n\t" \
    "v_cvt_pk_bf16_f32 v17, v18, v19\n\t" \
    "v_cvt_pk_bf16_f32 v18, v20, v21\n\t" \
    "v_cvt_pk_bf16_f32 v19, v22, v23\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[240:243], a[176:179], v[112:127]\n\t" \
    "v_exp_f32 v24, v24\n\t" \
    "v_exp_f32 v25, v25\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[244:247], a[180:183], v[48:63]\n\t" \
    "v_exp_f32 v26, v26\n\t" \
    "v_exp_f32 v27, v27\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[248:251], a[184:187], v[48:63]\n\t" \
    "v_exp_f32 v28, v28\n\t" \
    "v_exp_f32 v29, v29\n\t" \
    "v_mfma_f32_32x32x16_bf16 v[48:63], a[252:255], a[188:191], v[48:63]\n\t" \
    "v_exp_f32 v30, v30\n\t" \
    "v_exp_f32 v31, v31\n\t" \
    "v_add_f32 v176, v176, v24\n\t" \
    "v_add_f32 v176, v176, v28\n\t" \
    "v_add_f32 v177, v177, v25\n\t" \
    "v_add_f32 v177, v177, v29\n\t" \
    "v_add_f32 v178, v178, v26\n\t" \
    "v_add_f32 v178, v178, v30\n\t" \
    "v_add_f32 v179, v179, v27\n\t" \
    "v_add_f32 v179, v179, v31\n\t" \
    "v_cvt_pk_bf16_f32 v24, v24, v25\n\t" \
    "v_cvt_pk_bf16_f32 v25, v26, v27\n\t" \
    "v_cvt_pk_bf16_f32 v26, v28, v29\n\t" \
    "v_cvt_pk_bf16_f32 v27, v30, v31\n\t" \
    "v_add_f32 v176, v176, v177\n\t" \
    "v_add_f32 v178, v178, v179\n\t" \
    "v_add_f32 v186, v176, v178\n\t" \
    "v_add_f32 v166, v166, v186\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v186\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_exp_f32 v32, v32\n\t" \
    "ds_read_b128 a[224:227], %[ka0] offset:8192\n\t" \
    "v_exp_f32 v33, v33\n\t" \
    "ds_read_b128 a[228:231], %[ka1] offset:8192\n\t" \
    "ds_read_b128 a[232:235], %[ka2] offset:8192\n\t" \
    "ds_read_b128 a[236:239], %[ka3] offset:8192\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[192:195], v[0:3], a[64:79]\n\t" \
    "v_exp_f32 v34, v34\n\t" \
    "v_exp_f32 v35, v35\n\t" \
    "ds_read_b128 a[240:243], %[ka0] offset:12288\n\t" \
    "ds_read_b128 a[244:247], %[ka1] offset:12288\n\t" \
    "ds_read_b128 a[248:251], %[ka2] offset:12288\n\t" \
    "ds_read_b128 a[252:255], %[ka3] offset:12288\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[196:199], v[8:11], a[64:79]\n\t" \
    "v_exp_f32 v36, v36\n\t" \
    "v_exp_f32 v37, v37\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[200:203], v[16:19], a[64:79]\n\t" \
    "v_exp_f32 v38, v38\n\t" \
    "v_exp_f32 v39, v39\n\t" \
    "v_add_f32 v180, v32, v36\n\t" \
    "v_add_f32 v181, v33, v37\n\t" \
    "v_add_f32 v182, v34, v38\n\t" \
    "v_add_f32 v183, v35, v39\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[64:79], a[204:207], v[24:27], a[64:79]\n\t" \
    "v_cvt_pk_bf16_f32 v32, v32, v33\n\t" \
    "v_cvt_pk_bf16_f32 v33, v34, v35\n\t" \
    "v_cvt_pk_bf16_f32 v34, v36, v37\n\t" \
    "v_cvt_pk_bf16_f32 v35, v38, v39\n\t" \
    "v_exp_f32 v40, v40\n\t" \
    "v_exp_f32 v41, v41\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[208:211], v[0:3], a[80:95]\n\t" \
    "v_exp_f32 v42, v42\n\t" \
    "v_exp_f32 v43, v43\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[212:215], v[8:11], a[80:95]\n\t" \
    "v_exp_f32 v44, v44\n\t" \
    "v_exp_f32 v45, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[216:219], v[16:19], a[80:95]\n\t" \
    "v_exp_f32 v46, v46\n\t" \
    "v_exp_f32 v47, v47\n\t" \
    "v_add_f32 v180, v180, v40\n\t" \
    "v_add_f32 v180, v180, v44\n\t" \
    "v_add_f32 v181, v181, v41\n\t" \
    "v_add_f32 v181, v181, v45\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[80:95], a[220:223], v[24:27], a[80:95]\n\t" \
    "v_add_f32 v182, v182, v42\n\t" \
    "v_add_f32 v182, v182, v46\n\t" \
    "v_add_f32 v183, v183, v43\n\t" \
    "v_add_f32 v183, v183, v47\n\t" \
    "v_cvt_pk_bf16_f32 v40, v40, v41\n\t" \
    "v_cvt_pk_bf16_f32 v41, v42, v43\n\t" \
    "v_cvt_pk_bf16_f32 v42, v44, v45\n\t" \
    "v_cvt_pk_bf16_f32 v43, v46, v47\n\t" \
    "s_sub_u32 %[cnt], %[cnt], 1\n\t" \
    "s_cmp_lg_u32 %[cnt], 0\n\t" \
    "s_cbranch_scc1 FA2HS_LOOP_%=\n\t" \
    "FA2HS_EPI_%=:\n\t" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
    "v_exp_f32 v48, v48\n\t" \
    "v_exp_f32 v49, v49\n\t" \
    "v_exp_f32 v50, v50\n\t" \
    "v_exp_f32 v51, v51\n\t" \
    "v_exp_f32 v52, v52\n\t" \
    "v_exp_f32 v53, v53\n\t" \
    "v_exp_f32 v54, v54\n\t" \
    "v_exp_f32 v55, v55\n\t" \
    "v_add_f32 v180, v180, v48\n\t" \
    "v_add_f32 v180, v180, v52\n\t" \
    "v_add_f32 v181, v181, v49\n\t" \
    "v_add_f32 v181, v181, v53\n\t" \
    "v_add_f32 v182, v182, v50\n\t" \
    "v_add_f32 v182, v182, v54\n\t" \
    "v_add_f32 v183, v183, v51\n\t" \
    "v_add_f32 v183, v183, v55\n\t" \
    "v_cvt_pk_bf16_f32 v48, v48, v49\n\t" \
    "v_cvt_pk_bf16_f32 v49, v50, v51\n\t" \
    "v_cvt_pk_bf16_f32 v50, v52, v53\n\t" \
    "v_cvt_pk_bf16_f32 v51, v54, v55\n\t" \
    "v_exp_f32 v56, v56\n\t" \
    "v_exp_f32 v57, v57\n\t" \
    "v_exp_f32 v58, v58\n\t" \
    "v_exp_f32 v59, v59\n\t" \
    "v_exp_f32 v60, v60\n\t" \
    "v_exp_f32 v61, v61\n\t" \
    "v_exp_f32 v62, v62\n\t" \
    "v_exp_f32 v63, v63\n\t" \
    "v_add_f32 v180, v180, v56\n\t" \
    "v_add_f32 v180, v180, v60\n\t" \
    "v_add_f32 v181, v181, v57\n\t" \
    "v_add_f32 v181, v181, v61\n\t" \
    "v_add_f32 v182, v182, v58\n\t" \
    "v_add_f32 v182, v182, v62\n\t" \
    "v_add_f32 v183, v183, v59\n\t" \
    "v_add_f32 v183, v183, v63\n\t" \
    "v_cvt_pk_bf16_f32 v56, v56, v57\n\t" \
    "v_cvt_pk_bf16_f32 v57, v58, v59\n\t" \
    "v_cvt_pk_bf16_f32 v58, v60, v61\n\t" \
    "v_cvt_pk_bf16_f32 v59, v62, v63\n\t" \
    "v_add_f32 v180, v180, v181\n\t" \
    "v_add_f32 v182, v182, v183\n\t" \
    "v_add_f32 v187, v180, v182\n\t" \
    "v_add_f32 v167, v167, v187\n\t" \
    "v_cmp_nge_f32 vcc, 0x46000000, v187\n\t" \
    "s_nop 0\n\t" \
    "s_or_b64 %[flg], %[flg], vcc\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[192:195], v[32:35], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[196:199], v[40:43], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[200:203], v[48:51], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[96:111], a[204:207], v[56:59], a[96:111]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[208:211], v[32:35], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[212:215], v[40:43], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[216:219], v[48:51], a[112:127]\n\t" \
    "v_mfma_f32_32x32x16_bf16 a[112:127], a[220:223], v[56:59], a[112:127]\n\t" \
    "s_barrier\n\t" \
    "ds_write_b128 %[oa], a[0:3] offset:0\n\t" \
    "ds_write_b128 %[oa], a[4:7] offset:32\n\t" \
    "ds_write_b128 %[oa], a[8:11] offset:64\n\t" \
    "ds_write_b128 %[oa], a[12:15] offset:96\n\t" \
    "ds_write_b128 %[oa], a[16:19] offset:128\n\t" \
    "ds_write_b128 %[oa], a[20:23] offset:160\n\t" \
    "ds_write_b128 %[oa], a[24:27] offset:192\n\t" \
    "ds_write_b128 %[oa], a[28:31] offset:224\n\t" \
    "ds_write_b128 %[oa], a[32:35] offset:8704\n\t" \
    "ds_write_b128 %[oa], a[36:39] offset:8736\n\t" \
    "ds_write_b128 %[oa], a[40:43] offset:8768\n\t" \
    "ds_write_b128 %[oa], a[44:47] offset:8800\n\t" \
    "ds_write_b128 %[oa], a[48:51] offset:8832\n\t" \
    "ds_write_b128 %[oa], a[52:55] offset:8864\n\t" \
    "ds_write_b128 %[oa], a[56:59] offset:8896\n\t" \
    "ds_write_b128 %[oa], a[60:63] offset:8928\n\t" \
    "ds_write_b128 %[oa], a[64:67] offset:17408\n\t" \
    "ds_write_b128 %[oa], a[68:71] offset:17440\n\t" \
    "ds_write_b128 %[oa], a[72:75] offset:17472\n\t" \
    "ds_write_b128 %[oa], a[76:79] offset:17504\n\t" \
    "ds_write_b128 %[oa], a[80:83] offset:17536\n\t" \
    "ds_write_b128 %[oa], a[84:87] offset:17568\n\t" \
    "ds_write_b128 %[oa], a[88:91] offset:17600\n\t" \
    "ds_write_b128 %[oa], a[92:95] offset:17632\n\t" \
    "ds_write_b128 %[oa], a[96:99] offset:26112\n\t" \
    "ds_write_b128 %[oa], a[100:103] offset:26144\n\t" \
    "ds_write_b128 %[oa], a[104:107] offset:26176\n\t" \
    "ds_write_b128 %[oa], a[108:111] offset:26208\n\t" \
    "ds_write_b128 %[oa], a[112:115] offset:26240\n\t" \
    "ds_write_b128 %[oa], a[116:119] offset:26272\n\t" \
    "ds_write_b128 %[oa], a[120:123] offset:26304\n\t" \
    "ds_write_b128 %[oa], a[124:127] offset:26336\n\t" \
    "v_mov_b32 %[om0], v160\n\t" \
    "v_mov_b32 %[ol0], v164\n\t" \
    "v_mov_b32 %[om1], v161\n\t" \
    "v_mov_b32 %[ol1], v165\n\t" \
    "v_mov_b32 %[om2], v162\n\t" \
    "v_mov_b32 %[ol2], v166\n\t" \
    "v_mov_b32 %[om3], v163\n\t" \
    "v_mov_b32 %[ol3], v167\n\t" \
    "s_waitcnt lgkmcnt(0)\n\t" \
    ""

#define FA2_HS4_OUTPUTS_D64 [om0] "=&v"(hs_m[0]), [om1] "=&v"(hs_m[1]), [om2] "=&v"(hs_m[2]), [om3] "=&v"(hs_m[3]), [ol0] "=&v"(hs_l[0]), [ol1] "=&v"(hs_l[1]), [ol2] "=&v"(hs_l[2]), [ol3] "=&v"(hs_l[3]), [flg] "=&s"(hs_flag), [cnt] "+s"(hs_cnt), [goff] "+s"(hs_goff)
#define FA2_HS4_INPUTS_D64 [ka0] "v"(hs_ka[0]), [ka1] "v"(hs_ka[1]), [ka2] "v"(hs_ka[2]), [ka3] "v"(hs_ka[3]), [va0_0] "v"(hs_va[0][0]), [va0_1] "v"(hs_va[0][1]), [va1_0] "v"(hs_va[1][0]), [va1_1] "v"(hs_va[1][1]), [vo0] "v"(hs_vo[0]), [vo1] "v"(hs_vo[1]), [lo] "v"(hs_lo), [oa] "v"(hs_oa), [rsk] "s"(hs_rsk), [rsv] "s"(hs_rsv), [qb] "s"(hs_qb)
#define FA2_HS4_CLOBBERS_D64 "v0", "v1", "v2", "v3", "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255", "vcc", "scc", "memory"
#define FA2_HS4_LDS_D64 139264

