#!/usr/bin/env node
/* Golden vectors of the column-pivoted QR family (rrqr_decomp, rrqr_decomp_full, rrqr_rank, rrqr_lstsq, solve) from the real
 * reference bundle. Inputs come from the repo's counter-based generator nd4_uniform (twin of nd4js_amd/rng.py) and the input
 * families of tests/families.py; only numbers (outputs, sampled entries, norms) are written, as .npy files plus their own
 * manifest.json under tests/golden/rrqr/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_rrqr.js          # all cases (~35 s, most of it 2048^2)
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
const OUT = path.join(ROOT, 'tests', 'golden', 'rrqr');
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
function fro(a) { let s = 0; for (let i = 0; i < a.length; i++) s += a[i] * a[i]; return Math.sqrt(s); }
function sample(typed, n, seed) {
  const idx = new Int32Array(n), val = new Float64Array(n);
  for (let i = 0; i < n; i++) { idx[i] = hashIdx(seed, i, typed.length); val[i] = typed[idx[i]]; }
  return [idx, val];
}

/* ---------- cases ---------- */
function caseDecomp(name, seed, shape, fam, full) {
  const A = input(seed, shape, fam);
  const [Q, R, P] = nd.la.rrqr_decomp(A);
  const t = {Q, R, P, rank: nd.la.rrqr_rank(R)};
  if (full) { const [Qf, Rf, Pf] = nd.la.rrqr_decomp_full(A); Object.assign(t, {Qf, Rf, Pf}); }
  record(name, {op: 'rrqr_decomp', seed, shape, family: fam}, t);
}
function caseLarge(name, seed, N) {
  const A = input(seed, [N, N], 'dense');
  const t0 = Date.now();
  const [Q, R, P] = nd.la.rrqr_decomp(A);
  const ms = Date.now() - t0;
  const diag = new Float64Array(N); for (let i = 0; i < N; i++) diag[i] = R.data[i * N + i];
  const [qi, qv] = sample(Q.data, 4096, seed + 11), [ri, rv] = sample(R.data, 4096, seed + 12);
  const rank = nd.la.rrqr_rank(R);
  record(name, {op: 'rrqr_decomp', seed, shape: [N, N], family: 'dense', sampled: true, js_ms: ms,
                fro_Q: fro(Q.data), fro_R: fro(R.data)},
         {P, Rdiag: [diag, [N]], Q_idx: [qi, [4096]], Q_val: [qv, [4096]], R_idx: [ri, [4096]], R_val: [rv, [4096]], rank});
}
function caseLstsq(name, seed, shape, fam, J) {
  const A = input(seed, shape, fam), N = shape[shape.length - 2];
  const y = new nd.NDArray(Int32Array.from([N, J]), fill(seed + 1000, N * J));
  const x = nd.la.rrqr_lstsq(nd.la.rrqr_decomp(A), y);
  record(name, {op: 'rrqr_lstsq', seed, shape, family: fam, J, y_seed: seed + 1000}, {x});
}
function caseSolve(name, seed, N, fam, J) {
  const A = input(seed, [N, N], fam);
  const y = new nd.NDArray(Int32Array.from([N, J]), fill(seed + 1000, N * J));
  const t0 = Date.now();
  let x, singular = false;
  try { x = nd.la.solve(A, y); } catch (e) {
    if (!(e instanceof nd.la.SingularMatrixSolveError)) throw e;
    x = e.x; singular = true;
  }
  record(name, {op: 'solve', seed, shape: [N, N], family: fam, J, y_seed: seed + 1000, singular, js_ms: Date.now() - t0}, {x});
}

caseDecomp('sq32', 701, [32, 32], 'dense', false);
caseDecomp('tall17x5', 702, [17, 5], 'dense', true);
caseDecomp('wide5x17', 703, [5, 17], 'dense', false);
caseDecomp('batch4x24', 704, [4, 24, 24], 'dense', false);
let s = 720;
for (const fam of ['dense', 'sparse10', 'zerorow', 'zerocol', 'rankdef', 'diag', 'triu'])
  for (const [M, N] of [[48, 48], [60, 40], [40, 60]])
    caseDecomp(`${fam}_${M}x${N}`, s++, [M, N], fam, fam === 'dense' && M > N);
caseDecomp('identity16', 760, [16, 16], 'identity', false);
caseDecomp('dupcols20x12', 761, [20, 12], 'dupcols', false);
caseDecomp('zero8x6', 762, [8, 6], 'zero', false);
caseDecomp('sq200', 770, [200, 200], 'dense', false);
caseDecomp('tall300x128', 771, [300, 128], 'dense', false);
caseDecomp('wide128x300', 772, [128, 300], 'dense', false);
for (const J of [1, 5]) {
  caseLstsq(`ls_tall_J${J}`, 780 + J, [60, 40], 'dense', J);
  caseLstsq(`ls_wide_J${J}`, 790 + J, [40, 60], 'dense', J);
  caseLstsq(`ls_rankdef_J${J}`, 800 + J, [48, 48], 'rankdef', J);
}
caseSolve('solve64', 810, 64, 'dense', 1);
caseSolve('solve_singular48', 811, 48, 'rankdef', 2);
caseSolve('solve1024', 812, 1024, 'dense', 1);
caseLarge('large1024', 820, 1024);
caseLarge('large2048', 821, 2048);
fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1));
