#!/usr/bin/env node
/* Golden vectors of det, slogdet, det_tri, slogdet_tri, rank, lstsq and norm (src/la/det.js, rank.js, lstsq.js, norm.js) from the
 * real reference bundle. Inputs come from the repo's counter-based generator nd4_uniform (twin of nd4js_amd/rng.py) and the
 * input families of tests/families.py, with a few hand-built matrices (permutations, -I, overflowing diagonals, non-finite
 * entries). Only numbers are written: the outputs, and the inputs themselves where they are small (hand-built ones always, generated ones up to 8192 entries; larger
 * ones are regenerated from seed, shape, family and scale in the tests), as .npy files plus their own manifest.json under
 * tests/golden/det/. A case whose reference call throws records the message instead of outputs.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_det.js          # all cases (~20 s, most of it slogdet 2048^2)
 *
 * Without ND4_REFERENCE the bundle is found through BASELINE.json's reference_path, as the node tests do.
 */
'use strict';
const fs = require('fs'), path = require('path');
const ROOT = path.join(__dirname, '..');
function referenceBundle() {
  if (process.env.ND4_REFERENCE) return process.env.ND4_REFERENCE;
  const base = JSON.parse(fs.readFileSync(path.join(ROOT, 'BASELINE.json')));
  return path.join(base.reference_path, 'dist', 'nd.js');
}
const nd = require(referenceBundle());
const OUT = path.join(ROOT, 'tests', 'golden', 'det');
fs.mkdirSync(OUT, {recursive: true});

/* ---------- the repo's counter-based generator (nd4js_amd/rng.py) ---------- */
function fmix32(h) {
  h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b);
  h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35);
  h ^= h >>> 16; return h >>> 0;
}
function nd4_uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0);
  const lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  const m = (hi >>> 5) * 67108864 + (lo >>> 6);
  return m * 2.220446049250313e-16 - 1.0;
}
function fill(seed, n) { const a = new Float64Array(n); for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i); return a; }
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }

/* ---------- tests/families.py, plus the special inputs of this family ---------- */
function applyFamily(fam, a, M, N, seed) {
  switch (fam) {
    case 'dense': break;
    case 'sparse10': for (let i = 0; i < a.length; i++) if (hashIdx(seed + 77, i, 10) === 0) a[i] = 0; break;
    case 'zerorow': { const r = hashIdx(seed + 78, 0, M); for (let j = 0; j < N; j++) a[r * N + j] = 0; break; }
    case 'zerocol': { const c = hashIdx(seed + 79, 0, N); for (let i = 0; i < M; i++) a[i * N + c] = 0; break; }
    case 'rankdef': {
      const rank = Math.max(1, Math.min(M, N) >> 1);
      for (let i = rank; i < M; i++) for (let j = 0; j < N; j++)
        a[i * N + j] = 0.5 * a[((i - rank) % rank) * N + j] - 0.25 * a[((i + 1) % rank) * N + j];
      break; }
    case 'diag': for (let i = 0; i < M; i++) for (let j = 0; j < N; j++) if (i !== j) a[i * N + j] = 0; break;
    case 'triu': for (let i = 0; i < M; i++) for (let j = 0; j < i && j < N; j++) a[i * N + j] = 0; break;
    case 'identity': for (let i = 0; i < M; i++) for (let j = 0; j < N; j++) a[i * N + j] = i === j ? 1 : 0; break;
    case 'zero': a.fill(0); break;
    case 'dupcols': for (let i = 0; i < M; i++) for (let j = 1; j < N; j += 2) a[i * N + j] = a[i * N + j - 1]; break;
    default: throw new Error(fam);
  }
  return a;
}
function input(seed, shape, fam) {
  const M = shape[shape.length - 2], N = shape[shape.length - 1], n = shape.reduce((a, b) => a * b, 1);
  const a = fill(seed, n);
  for (let o = 0, b = 0; o < n; o += M * N, b++) applyFamily(fam, a.subarray(o, o + M * N), M, N, seed + b);
  return new nd.NDArray(Int32Array.from(shape), a);
}

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape) {
  const descr = typed instanceof Float64Array ? '<f8' : typed instanceof Int32Array ? '<i4' : null;
  if (!descr) throw new Error('dtype');
  let hdr = `{'descr': '${descr}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  fs.writeFileSync(path.join(OUT, name + '.npy'), Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]));
}
const manifest = {rng: 'fmix32-v1', cases: {}};
function record(name, meta, tensors) {
  const files = {};
  for (const [k, arr] of Object.entries(tensors)) {
    const [typed, shape] = arr instanceof nd.NDArray ? [arr.data, Array.from(arr.shape)] : arr;
    npy(`${name}.${k}`, typed, shape); files[k] = `${name}.${k}.npy`;
  }
  manifest.cases[name] = Object.assign({}, meta, {files});
  console.log('wrote', name);
}
function lowrank(seed, M, N, r) {                       // B [M, r] C [r, N] from the generator
  const B = fill(seed, M * r), C = fill(seed + 1, r * N), a = new Float64Array(M * N);
  for (let i = 0; i < M; i++) for (let k = 0; k < r; k++) { const b = B[i * r + k]; for (let j = 0; j < N; j++) a[i * N + j] += b * C[k * N + j]; }
  return new nd.NDArray(Int32Array.from([M, N]), a);
}

const SMALL = 8192;
const arr = (shape, data) => new nd.NDArray(Int32Array.from(shape), Float64Array.from(data));
function gen(seed, shape, fam, scale) {
  const A = input(seed, shape, fam);
  if (scale !== undefined && scale !== 1) for (let i = 0; i < A.data.length; i++) A.data[i] *= scale;
  return A;
}
function run(f) { try { return {out: f()}; } catch (e) { return {error: e.message}; } }
// ops: a list of 'det', 'slogdet', 'det_tri', 'slogdet_tri', 'norm', 'rank', 'lstsq'
function caseOf(name, meta, A, ops, y) {
  const tensors = {}, results = {}, stored = meta.seed === undefined || A.data.length <= SMALL;   // hand-built inputs: always
  if (stored) tensors.A = A;
  if (y) tensors.y = y;
  for (const op of ops) {
    const t0 = Date.now();
    const r = run(() => op === 'lstsq' ? nd.la.lstsq(A, y) : nd.la[op](A));
    const ms = Date.now() - t0;
    if (r.error !== undefined) { results[op] = {error: r.error}; continue; }
    results[op] = {js_ms: ms};
    if (op === 'norm') results[op].value = r.out === r.out ? (isFinite(r.out) ? r.out : String(r.out)) : 'NaN';
    if (op === 'norm') tensors[op] = [Float64Array.of(r.out), []];
    else if (op === 'slogdet' || op === 'slogdet_tri') { tensors[op + '_sign'] = r.out[0]; tensors[op + '_logdet'] = r.out[1]; }
    else if (op === 'rank') tensors[op] = [Int32Array.from(r.out.data), Array.from(r.out.shape)];
    else tensors[op] = r.out;
  }
  record(name, Object.assign({shape: Array.from(A.shape), ops: results, stored_input: stored}, meta), tensors);
}
const gcase = (name, seed, shape, fam, ops, scale) => caseOf(name, {seed, family: fam, scale: scale === undefined ? 1 : scale}, gen(seed, shape, fam, scale), ops);
const DET = ['det', 'slogdet'];

// ---- small tier (one lane per matrix) and wave tier (one wave per matrix); random signs come with the uniform [-1, 1) entries
let s = 1000;
for (const [b, n] of [[64, 1], [512, 2], [1024, 3], [4096, 4], [256, 7], [256, 8]]) gcase(`small_${b}x${n}`, s++, [b, n, n], 'dense', DET);
for (const [b, n] of [[32, 9], [16, 16], [8, 33], [4, 64], [2, 48]]) gcase(`wave_${b}x${n}`, s++, [b, n, n], 'dense', DET);
for (const fam of ['sparse10', 'zerorow', 'zerocol', 'rankdef', 'triu', 'diag']) { gcase(`${fam}_8`, s++, [16, 8, 8], fam, DET); gcase(`${fam}_40`, s++, [3, 40, 40], fam, DET); }
// ---- large tier (R-only QR): det overflows beyond ~ 300^2, slogdet stays finite
gcase('large_65', s++, [65, 65], 'dense', DET);
gcase('large_128', s++, [128, 128], 'dense', DET);
gcase('large_512', s++, [512, 512], 'dense', DET);
gcase('large_1024', s++, [1024, 1024], 'dense', DET);
gcase('large_2048', s++, [2048, 2048], 'dense', ['slogdet']);
gcase('large_rankdef_96', s++, [96, 96], 'rankdef', DET);
// ---- known signs, singular and degenerate
function wellcond(seed, n) { const A = gen(seed, [n, n], 'dense'); for (let i = 0; i < n; i++) A.data[i * n + i] += (A.data[i * n + i] >= 0 ? n : -n); return A; }
function swapRows(A, i, j) { const n = A.shape[1]; for (let k = 0; k < n; k++) { const t = A.data[i * n + k]; A.data[i * n + k] = A.data[j * n + k]; A.data[j * n + k] = t; } return A; }
function perm(n, seed) { const p = Array.from({length: n}, (_, i) => i); for (let i = n - 1; i > 0; i--) { const j = hashIdx(seed, i, i + 1); [p[i], p[j]] = [p[j], p[i]]; }
                          const a = new Float64Array(n * n); p.forEach((c, r) => { a[r * n + c] = 1; }); return arr([n, n], a); }
const eye = (n, v) => { const a = new Float64Array(n * n); for (let i = 0; i < n; i++) a[i * n + i] = v; return arr([n, n], a); };
caseOf('wellcond_6', {}, wellcond(s++, 6), DET);
caseOf('rowswap_6', {}, swapRows(wellcond(s - 1, 6), 1, 4), DET);
caseOf('rowswap_20', {}, swapRows(wellcond(s++, 20), 0, 19), DET);
caseOf('rowswap_80', {}, swapRows(wellcond(s++, 80), 3, 70), DET);
caseOf('perm_10', {}, perm(10, s++), DET);
caseOf('perm_64', {}, perm(64, s++), DET);
caseOf('negeye_5', {}, eye(5, -1), DET);
caseOf('negeye_70', {}, eye(70, -1), DET);
caseOf('eye_3', {}, eye(3, 1), DET);
caseOf('eye_40', {}, eye(40, 1), DET);
caseOf('zero_4', {}, eye(4, 0), DET);
caseOf('zero_12', {}, eye(12, 0), DET);
function duprows(seed, n) { const A = gen(seed, [n, n], 'dense'); for (let k = 0; k < n; k++) A.data[(n - 1) * n + k] = A.data[k]; return A; }
caseOf('duprows_6', {}, duprows(s++, 6), DET);
caseOf('duprows_20', {}, duprows(s++, 20), DET);
caseOf('duprows_100', {}, duprows(s++, 100), DET);
// ---- tall (qr_decomp's N x N R with the c >= 0 signs) and wide (det_tri's error)
gcase('tall_60x40', s++, [60, 40], 'dense', DET);
gcase('tall_5x9x4', s++, [5, 9, 4], 'dense', DET);
gcase('tall_1000x700', s++, [1000, 700], 'dense', ['slogdet']);
gcase('wide_3x5', s++, [3, 5], 'dense', DET);
// ---- overflow / underflow of the product in index order, with a finite slogdet
function bigdiag(n, vals) { const a = new Float64Array(n * n); for (let i = 0; i < n; i++) { a[i * n + i] = vals[i % vals.length]; if (i + 1 < n) a[i * n + i + 1] = 0.5; } return arr([n, n], a); }
caseOf('overflow_8', {}, bigdiag(8, [1e200, 1e200, 1e-200, -1e-150]), DET.concat(['det_tri', 'slogdet_tri']));
caseOf('underflow_8', {}, bigdiag(8, [1e-200, 1e-200, 1e200, 3]), DET.concat(['det_tri', 'slogdet_tri']));
caseOf('overflow_40', {}, bigdiag(40, [1e100, -1e90, 1e80]), DET.concat(['det_tri', 'slogdet_tri']));
gcase('scaled_1e30_30', s++, [30, 30], 'dense', DET, 1e30);
gcase('scaled_1e-30_100', s++, [100, 100], 'dense', DET, 1e-30);
// ---- non-finite entries: a rotation that meets them makes the reference assert; the diagonal rule takes them as they are
function edit(A, edits) { for (const [i, v] of edits) A.data[i] = v; return A; }
caseOf('nan_4', {}, edit(gen(s++, [4, 4], 'dense'), [[9, NaN]]), DET);
caseOf('inf_4', {}, edit(gen(s++, [4, 4], 'dense'), [[5, Infinity]]), DET);
caseOf('nan_20', {}, edit(gen(s++, [20, 20], 'dense'), [[77, NaN]]), DET);
caseOf('triu_nan_diag_5', {}, edit(gen(s++, [5, 5], 'triu'), [[12, NaN]]), DET.concat(['det_tri', 'slogdet_tri']));
caseOf('triu_inf_upper_5', {}, edit(gen(s++, [5, 5], 'triu'), [[3, -Infinity]]), DET.concat(['det_tri', 'slogdet_tri']));
caseOf('signed_zero_diag', {}, arr([4, 3, 3], [-0, 1, 2, 0, 2, 3, 0, 0, 4,   0, 1, 2, 0, -2, 3, 0, 0, 4,   -0, 1, 2, 0, -0, 3, 0, 0, -4,   1, 0, 0, 0, -1, 0, 0, 0, NaN]),
       ['det_tri', 'slogdet_tri']);
// ---- det_tri / slogdet_tri on triangular and general input (only the diagonal is read)
gcase('tri_triu_5x6', s++, [5, 6, 6], 'triu', ['det_tri', 'slogdet_tri']);
gcase('tri_dense_5x6', s++, [5, 6, 6], 'dense', ['det_tri', 'slogdet_tri']);
gcase('tri_dense_300', s++, [300, 300], 'dense', ['det_tri', 'slogdet_tri']);
gcase('tri_dense_1000x16', s++, [1000, 16, 16], 'dense', ['det_tri', 'slogdet_tri']);
// ---- norm
gcase('norm_2048', s++, [2048, 2048], 'dense', ['norm']);
gcase('norm_1e300', s++, [100, 100], 'dense', ['norm'], 1e300);
gcase('norm_1e-300', s++, [100, 100], 'dense', ['norm'], 1e-300);
caseOf('norm_inf', {}, edit(gen(s++, [50, 50], 'dense'), [[1234, -Infinity]]), ['norm']);
caseOf('norm_nan', {}, edit(gen(s++, [50, 50], 'dense'), [[17, NaN]]), ['norm']);
caseOf('norm_nan_inf', {}, edit(gen(s++, [50, 50], 'dense'), [[17, NaN], [2000, Infinity]]), ['norm']);
caseOf('norm_inf_nan', {}, edit(gen(s++, [50, 50], 'dense'), [[17, Infinity], [2000, NaN]]), ['norm']);
caseOf('norm_vector', {}, arr([7], [3, -4, 0, 1e-310, 12, -0, 2]), ['norm']);
// ---- rank / lstsq on low-rank input with a clear singular-value gap
function lowrankB(seed, lead, M, N, r) {
  const a = new Float64Array(lead * M * N);
  for (let b = 0; b < lead; b++) { const L = lowrank(seed + 2 * b, M, N, r); a.set(L.data, b * M * N); }
  return arr(lead > 1 ? [lead, M, N] : [M, N], a);
}
for (const [name, lead, M, N, r] of [['lowrank_40x30_r12', 1, 40, 30, 12], ['lowrank_100x80_r25', 1, 100, 80, 25], ['lowrank_30x50_r7', 1, 30, 50, 7],
                                       ['lowrank_3x20x15_r5', 3, 20, 15, 5], ['fullrank_24x16', 1, 24, 16, 16]]) {
  const seed = s; s += 8;
  const A = lowrankB(seed, lead, M, N, r);
  const y = arr([M, 3], fill(seed + 100, M * 3));
  caseOf(name, {lowrank: r, seed}, A, ['rank', 'lstsq'], y);
}
fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
