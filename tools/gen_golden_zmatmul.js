#!/usr/bin/env node
/* Golden vectors of the complex matmul2 pairings (src/la/matmul.js:74-87: matmul2_CC, matmul2_CR, matmul2_RC) from the real
 * reference bundle. Inputs come from the repo's counter-based generator nd4_uniform (twin of nd4js_amd/rng.py): a complex
 * operand is the interleaved buffer fill(seed, 2 numel), a float64 one fill(seed, numel), an int32 one trunc(1000 fill(seed,
 * numel)). Hand-built inputs (non-finite entries, cancelling real parts) are always stored, generated ones only where they are
 * small; the tests regenerate the others from seed and shape. For large products only some rows of C are stored: the reference's
 * rows do not depend on each other, so matmul2(A[rows], B) is its answer for those rows. Only numbers are written, as .npy
 * files (complex as <c16) plus their own manifest.json under tests/golden/zmatmul/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_zmatmul.js          # all cases (~10 s)
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
const OUT = path.join(ROOT, 'tests', 'golden', 'zmatmul');
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

const numel = shape => shape.reduce((a, b) => a * b, 1);
// dtype: 'complex128' | 'float64' | 'int32'
function operand(dtype, shape, data) {
  const n = numel(shape);
  if (dtype === 'complex128') return new nd.NDArray(Int32Array.from(shape), new nd.dt.Complex128Array(data.buffer, data.byteOffset, n));
  return new nd.NDArray(Int32Array.from(shape), data);
}
function generated(dtype, seed, shape) {
  const n = numel(shape);
  if (dtype === 'complex128') return fill(seed, 2 * n);
  if (dtype === 'float64') return fill(seed, n);
  return Int32Array.from(fill(seed, n), u => Math.trunc(u * 1000));
}
const storage = a => a.dtype === 'complex128' ? a.data._array : a.data;

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape, complex) {
  const descr = complex ? '<c16' : typed instanceof Float64Array ? '<f8' : typed instanceof Int32Array ? '<i4' : null;
  if (!descr) throw new Error('dtype');
  let hdr = `{'descr': '${descr}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  fs.writeFileSync(path.join(OUT, name + '.npy'), Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]));
  return name + '.npy';
}
const manifest = {rng: 'fmix32-v1', int32: 'trunc(1000 u)', cases: {}};
const SMALL = 8192;   // doubles: generated inputs up to this size are stored as well

// one case: operands {dtype, shape, seed} (generated) or {dtype, shape, data} (hand-built); rows: null = all of C
function zcase(name, opA, opB, rows, extra) {
  const meta = Object.assign({}, extra || {});
  const ops = [];
  for (const [key, op] of [['A', opA], ['B', opB]]) {
    const data = op.data || generated(op.dtype, op.seed, op.shape);
    const m = {dtype: op.dtype, shape: op.shape};
    if (op.seed !== undefined) m.seed = op.seed;
    if (op.seed === undefined || data.length <= SMALL) m.file = npy(`${name}.${key}`, data, op.shape, op.dtype === 'complex128');
    meta[key] = m;
    ops.push(operand(op.dtype, op.shape, data));
  }
  let [A, B] = ops;
  if (rows) {            // the reference's own rows: matmul2 of the selected rows of A (2-D A only)
    const K = opA.shape[1], e = opA.dtype === 'complex128' ? 2 : 1, src = storage(A);
    const sub = src instanceof Int32Array ? new Int32Array(rows.length * K * e) : new Float64Array(rows.length * K * e);
    rows.forEach((r, i) => sub.set(src.subarray(r * K * e, (r + 1) * K * e), i * K * e));
    A = operand(opA.dtype, [rows.length, K], sub);
    meta.rows = npy(`${name}.rows`, Int32Array.from(rows), [rows.length]);
  }
  const t0 = Date.now();
  const C = nd.la.matmul2(A, B);
  meta.js_ms = Date.now() - t0;
  if (C.dtype !== 'complex128') throw new Error(`${name}: reference returned ${C.dtype}`);
  meta.C = npy(`${name}.C`, C.data._array, Array.from(C.shape), true);
  meta.shape = Array.from(C.shape);
  manifest.cases[name] = meta;
  console.log('wrote', name, meta.js_ms + ' ms');
}

const Z = 'complex128', R = 'float64', N = 'int32';
const PAIRS = {CC: [Z, Z], CR: [Z, R], RC: [R, Z], CI: [Z, N], IC: [N, Z]};
let s = 5000;
// ---- every pairing at an odd shape, and the extents around the tile (128 x 64 complex, K-step 8)
for (const [p, [da, db]] of Object.entries(PAIRS)) zcase(`pair_${p}`, {dtype: da, shape: [37, 29], seed: s++}, {dtype: db, shape: [29, 45], seed: s++}, null, {pairing: p});
for (const [p, [da, db]] of Object.entries(PAIRS).slice(0, 3)) {
  for (const [I, K, J] of [[1, 1, 1], [5, 1, 7], [130, 19, 70], [128, 16, 64], [257, 13, 65], [64, 40, 3]])
    zcase(`odd_${p}_${I}x${K}x${J}`, {dtype: da, shape: [I, K], seed: s++}, {dtype: db, shape: [K, J], seed: s++}, null, {pairing: p});
}
// ---- broadcast leading axes
for (const [p, [da, db]] of Object.entries(PAIRS)) zcase(`bcast_${p}`, {dtype: da, shape: [2, 1, 9, 11], seed: s++}, {dtype: db, shape: [3, 11, 10], seed: s++}, null, {pairing: p});
zcase('bcast_CC_left', {dtype: Z, shape: [12, 8], seed: s++}, {dtype: Z, shape: [4, 1, 8, 6], seed: s++}, null, {pairing: 'CC'});
// ---- real parts that cancel: Ai = Ar and Bi = Br make every Ar Br - Ai Bi an exact zero; then a near-cancelling perturbation
{
  const I = 24, K = 33, J = 17, a = fill(s++, I * K), b = fill(s++, K * J);
  const A = new Float64Array(2 * I * K), B = new Float64Array(2 * K * J);
  for (let i = 0; i < I * K; i++) { A[2 * i] = a[i]; A[2 * i + 1] = a[i]; }
  for (let i = 0; i < K * J; i++) { B[2 * i] = b[i]; B[2 * i + 1] = b[i]; }
  zcase('cancel_exact', {dtype: Z, shape: [I, K], data: A}, {dtype: Z, shape: [K, J], data: B}, null, {pairing: 'CC'});
  const A2 = Float64Array.from(A), e = fill(s++, I * K);
  for (let i = 0; i < I * K; i++) A2[2 * i + 1] += 1e-9 * e[i];
  zcase('cancel_near', {dtype: Z, shape: [I, K], data: A2}, {dtype: Z, shape: [K, J], data: B}, null, {pairing: 'CC'});
}
// ---- non-finite entries in each operand, every pairing: NaN / Inf must land where the reference puts them
{
  const I = 6, K = 5, J = 7;
  const specials = (dtype, shape, seed, marks) => {
    const d = generated(dtype === N ? R : dtype, seed, shape);
    for (const [idx, v] of marks) d[idx % d.length] = v;
    return d;
  };
  // entries chosen so that single Infs, Inf - Inf, Inf * 0 and NaN all occur, in the real and in the imaginary parts
  const mA = [[0, Infinity], [13, -Infinity], [22, NaN], [31, Infinity], [41, 0]];
  const mB = [[3, Infinity], [16, NaN], [27, -Infinity], [44, Infinity], [50, 0]];
  for (const p of ['CC', 'CR', 'RC']) {
    const [da, db] = PAIRS[p];
    const A = specials(da, [I, K], s++, mA), B = specials(db, [K, J], s++, mB);
    zcase(`special_${p}`, {dtype: da, shape: [I, K], data: A}, {dtype: db, shape: [K, J], data: B}, null, {pairing: p});
    // Inf in one operand only, multiplied by finite nonzero entries: (inf + 0i) * 1 stays inf + 0i for CR / RC
    const A1 = specials(da, [I, K], s++, [[0, Infinity]]), B1 = generated(db, s++, [K, J]);
    if (da === Z) A1[1] = 0;
    zcase(`special_${p}_inf_only`, {dtype: da, shape: [I, K], data: A1}, {dtype: db, shape: [K, J], data: B1}, null, {pairing: p});
  }
}
// ---- large products as sampled rows: 4096^2 CC and CR; one I >= 1500 product (the host form's row-split pipeline runs in chunks)
const sample = (I, n, seed) => Array.from({length: n}, (_, i) => (i === 0 ? 0 : i === n - 1 ? I - 1 : fmix32((seed + Math.imul(i, 0x9E3779B1)) >>> 0) % I))
  .filter((v, i, a) => a.indexOf(v) === i).sort((x, y) => x - y);
zcase('large_CC_4096', {dtype: Z, shape: [4096, 4096], seed: 7001}, {dtype: Z, shape: [4096, 4096], seed: 7002}, sample(4096, 6, 7003), {pairing: 'CC'});
zcase('large_CR_4096', {dtype: Z, shape: [4096, 4096], seed: 7011}, {dtype: R, shape: [4096, 4096], seed: 7012}, sample(4096, 6, 7013), {pairing: 'CR'});
zcase('rows_CC_2000', {dtype: Z, shape: [2000, 3000], seed: 7021}, {dtype: Z, shape: [3000, 2500], seed: 7022}, sample(2000, 8, 7023), {pairing: 'CC'});

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
console.log('manifest:', Object.keys(manifest.cases).length, 'cases');
