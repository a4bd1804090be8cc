#!/usr/bin/env node
/* Golden vectors of the NDArray core's data movement from the real reference bundle: sliceElems (src/nd_array.js:531-642),
 * transpose(...axes) (src/nd_array.js:375-436), reshape (src/nd_array.js:438-462), nd.concat (src/concat.js) and nd.stack
 * (src/stack.js), on float64, int32 and complex128 arrays.
 * Inputs come from the repo's counter-based generator nd4_uniform(seed, idx) (twin of nd4js_amd/rng.py); float64 and complex128
 * inputs have a NaN with a payload and -0 (float64 only: the reference's Complex refuses the one and rewrites the other),
 * +Infinity, -Infinity and two denormals planted at hashed positions, int32 inputs the extreme values. Every input and every result is stored (complex128 as
 * <c16). A refused call stores nothing but its exact message under `errors`, with the shapes and arguments that repeat it. A
 * slice is written as the reference takes it, with null for an omitted entry of [start, end, step]. Only numbers and recorded texts are written: .npy files plus manifest.json (with
 * the sha256 of every file) under tests/golden/slice/, every file below 100 KB.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_slice.js
 *
 * Without ND4_REFERENCE the bundle is found through BASELINE.json's reference_path, as the node tests do.
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const ROOT = path.join(__dirname, '..');
function referenceBundle() {
  if (process.env.ND4_REFERENCE) return process.env.ND4_REFERENCE;
  const base = JSON.parse(fs.readFileSync(path.join(ROOT, 'BASELINE.json')));
  return path.join(base.reference_path, 'dist', 'nd.js');
}
const nd = require(referenceBundle());
const OUT = path.join(ROOT, 'tests', 'golden', 'slice');
fs.mkdirSync(OUT, {recursive: true});
for (const f of fs.readdirSync(OUT)) if (f.endsWith('.npy')) fs.unlinkSync(path.join(OUT, f));
const LIMIT = 100 * 1000;

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
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed >>> 0) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }
const prod = s => s.reduce((a, b) => a * b, 1);
// [high word, low word]: a quiet NaN with a payload, +Infinity, -Infinity, -0, the smallest denormal, a negative denormal
const SPECIAL_WORDS = [[0x7ff8dead, 0x0000beef], [0x7ff00000, 0], [0xfff00000, 0], [0x80000000, 0], [0, 1], [0x80012345, 0x6789abcd]];
// The reference reads and stores a complex element through `new Complex(z)`, which refuses a NaN part and whose `z.im || 0`
// turns a -0 part into +0: that is its conversion, not a move, so complex inputs (forComplex) carry neither of the two.
function fillDoubles(seed, n, forComplex) {
  const a = new Float64Array(n), w = new Uint32Array(a.buffer);
  for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i);
  if (n >= 12) SPECIAL_WORDS.filter((w, q) => !(forComplex && (q === 0 || q === 3))).forEach(([hi, lo], q) => { const p = hashIdx(seed, q, n); w[2 * p] = lo; w[2 * p + 1] = hi; });
  return a;
}
function fillInts(seed, n) {
  const a = Int32Array.from({length: n}, (_, i) => Math.trunc(nd4_uniform(seed, i) * 1e9));
  if (n >= 12) [-2147483648, 2147483647, 0, -1].forEach((v, q) => { a[hashIdx(seed, q, n)] = v; });
  return a;
}

/* ---------- npy + manifest ---------- */
const DESCR = {float64: '<f8', int32: '<i4', complex128: '<c16'};
const storage = a => a.dtype === 'complex128' ? a.data._array : a.data;
function npy(file, typed, shape, dtype) {
  let hdr = `{'descr': '${DESCR[dtype]}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > LIMIT) throw new Error(file + ': larger than ' + LIMIT + ' bytes');
  fs.writeFileSync(path.join(OUT, file), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', inputs: {}, cases: {}, errors: []};
function entry(name, a) {
  const shape = Array.from(a.shape), file = name + '.npy';
  if (!DESCR[a.dtype]) throw new Error(name + ': the reference returned dtype ' + a.dtype);
  return {file, shape, dtype: a.dtype, sha256: npy(file, storage(a), shape, a.dtype)};
}
const INPUT = {};
const PREFIX = {float64: 'A', int32: 'I', complex128: 'Z'};
let seed = 47000;
// one input per (dtype, shape, tag)
function input(dtype, shape, tag) {
  const name = `${PREFIX[dtype]}${tag || ''}_${shape.join('x')}`;
  if (INPUT[name]) return name;
  const n = prod(shape), s = seed++;
  let a;
  if (dtype === 'complex128') a = new nd.NDArray(Int32Array.from(shape), new nd.dt.Complex128Array(fillDoubles(s, 2 * n, true).buffer, 0, n));
  else a = new nd.NDArray(Int32Array.from(shape), dtype === 'int32' ? fillInts(s, n) : fillDoubles(s, n));
  INPUT[name] = a;
  manifest.inputs[name] = entry(name, a);
  return name;
}
let count = 0;
function golden(name, fn, args, result) {
  if (manifest.cases[name]) throw new Error('duplicate case ' + name);
  manifest.cases[name] = Object.assign({fn}, args, {out: entry(name + '.out', result)});
  count++;
}
const undef = s => Array.isArray(s) ? s.map(x => x === null ? undefined : x) : s;
const serial = {};
const tagOf = key => { serial[key] = (serial[key] || 0) + 1; return String(serial[key]).padStart(2, '0'); };
const DTYPES = ['float64', 'int32', 'complex128'];

/* ---------- sliceElems ---------- */
function sliceCase(dtype, shape, slices) {
  const a = input(dtype, shape);
  golden(`slice_${a}_${tagOf('s' + a)}`, 'sliceElems', {A: a, slices}, INPUT[a].sliceElems(...slices.map(undef)));
}
const SMALL_SLICES = [
  [], ['...'], ['...', [null, null, -1]], ['...', [5, 0, -2]], [-1], [1, 2], ['new', 1, 'new'], [[1, 3]], [[1, 3], [2, 5]], [[-3, -1], [-4, null]],
  ['...', 0], [[null, null, 2], [null, null, 3]], [[3, null, -1], [4, null, -2]], [[null, 2, -1]], ['...', 'new'], [2, 'new', '...'], [[0, 4, 3], -2],
];
for (const dtype of DTYPES) for (const s of SMALL_SLICES) sliceCase(dtype, [4, 6], s);
// rows: lengths, offsets and pitches that allow 16-byte words, 8-byte words or single words only; stepped and reversed axes
const ROW_SLICES = [
  [[3, 60], [2, 130]], [[3, 60], [2, 129]], [[3, 60], [3, 129]], ['...', [5, 6]], [[null, null, 3]], [[null, null, -1]],
  ['...', [null, null, 2]], ['...', [null, null, -1]], ['...', [129, 0, -3]], [[null, null, -2], [null, null, -1]], [[3, 60], [4, 128]],
];
for (const s of ROW_SLICES) { sliceCase('float64', [67, 130], s); sliceCase('int32', [67, 130], s); }
for (const s of [[[3, 30], [2, 36]], [[3, 30], [1, 36]], ['...', [5, 6]], [[null, null, -1]], ['...', [null, null, -2]]]) sliceCase('complex128', [33, 37], s);
for (const dtype of DTYPES) {
  sliceCase(dtype, [3, 2, 17, 30], ['...', 1, [3, 16], [2, 30]]);
  sliceCase(dtype, [3, 2, 17, 30], [2]);
  sliceCase(dtype, [3, 2, 17, 30], [[null, null, -1], '...', [1, 29, 3]]);
  sliceCase(dtype, [33], [[30, 2, -3]]);
  sliceCase(dtype, [33], [7]);
}
// 8 axes that cannot be merged, and 10 axes (more than one launch takes)
const step2 = n => Array.from({length: n}, () => [null, null, 2]);
sliceCase('float64', [2, 3, 2, 3, 2, 3, 2, 5], step2(8));
sliceCase('int32', [2, 3, 2, 3, 2, 3, 2, 5], step2(8));
sliceCase('float64', [3, 3, 3, 3, 3, 3, 3, 3, 3, 3].map((x, i) => i < 4 ? 2 : 3), step2(10));
sliceCase('float64', [2, 2, 2, 2, 2, 2, 2, 2, 2, 2], [[null, null, -1], 1, '...', 0, [null, null, -1]]);

/* ---------- transpose(...axes) ---------- */
function transposeCase(dtype, shape, axes) {
  const a = input(dtype, shape);
  golden(`transpose_${a}_${tagOf('t' + a)}`, 'transpose', {A: a, axes}, INPUT[a].transpose(...axes));
}
const PERM3 = [[], [0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0], [2, 0], [1], [2]];
for (const dtype of DTYPES) {
  for (const axes of PERM3) transposeCase(dtype, [5, 17, 19], axes);
  transposeCase(dtype, [4, 6], [1, 0]);
  transposeCase(dtype, [33], [0]);
  transposeCase(dtype, [2, 3, 4, 5], [3, 1, 0, 2]);
}
transposeCase('float64', [2, 3, 4], [2, 0]);
for (const axes of [[2, 0, 1], [1, 2, 0]]) { transposeCase('float64', [3, 63, 64], axes); transposeCase('int32', [2, 65, 67], axes); }
transposeCase('float64', [35, 33, 4], [1, 0, 2]);
transposeCase('complex128', [65, 34], [1, 0]);
transposeCase('float64', [2, 3, 2, 3, 2, 3, 2, 5], [7, 6, 5, 4, 3, 2, 1, 0]);

/* ---------- reshape ---------- */
for (const dtype of DTYPES) for (const shape of [[-1, 3], [24], [2, 3, 4], [1, 24, 1], [6, -1], [-1]]) {
  const a = input(dtype, [4, 6]);
  golden(`reshape_${a}_${tagOf('r' + a)}`, 'reshape', {A: a, shape}, INPUT[a].reshape(...shape));
}

/* ---------- concat / stack ---------- */
function listCase(fn, dtype, axis, shapes, tag) {
  const names = shapes.map((s, k) => input(dtype, s, 'c' + k));
  const arrays = names.map(n => INPUT[n]);
  const result = axis === null ? nd[fn](arrays) : nd[fn](axis, arrays);
  golden(`${fn}_${PREFIX[dtype]}_${tag}_ax${axis === null ? 'none' : axis}`, fn, {arrays: names, axis}, result);
}
for (const dtype of DTYPES) {
  listCase('concat', dtype, 0, [[5, 7]], 'one');
  listCase('concat', dtype, null, [[5, 7], [3, 7]], 'two');
  listCase('concat', dtype, 0, [[5, 7], [3, 7], [1, 7], [2, 7], [4, 7]], 'five');
  listCase('concat', dtype, 1, [[9, 3], [9, 64], [9, 1]], 'cols');
  listCase('concat', dtype, -1, [[9, 3], [9, 64], [9, 1]], 'cols');
  listCase('concat', dtype, 2, [[2, 3, 4, 5], [2, 3, 1, 5], [2, 3, 2, 5]], 'mid');
  listCase('concat', dtype, -3, [[2, 3, 4, 5], [2, 1, 4, 5]], 'mid');
  listCase('concat', dtype, 0, [[6], [1], [9]], 'vec');
  listCase('stack', dtype, 0, [[5, 7]], 'one');
  listCase('stack', dtype, null, [[5, 7], [5, 7]], 'two');
  listCase('stack', dtype, 1, [[5, 7], [5, 7], [5, 7], [5, 7], [5, 7]], 'five');
  listCase('stack', dtype, 2, [[5, 7], [5, 7]], 'last');
  listCase('stack', dtype, -1, [[5, 7], [5, 7], [5, 7]], 'last');
  listCase('stack', dtype, 2, [[2, 3, 4, 5], [2, 3, 4, 5]], 'mid');
  listCase('stack', dtype, -2, [[6], [6]], 'vec');
}

/* ---------- refused calls: the exact messages ---------- */
function refused(fn, how, call) {
  let message = null;
  try { call(); } catch (e) { message = e.message; }
  if (message === null) throw new Error(`${fn} ${JSON.stringify(how)}: expected the reference to throw`);
  manifest.errors.push(Object.assign({fn, message}, how));
}
const zeros = shape => new nd.NDArray(Int32Array.from(shape), new Float64Array(prod(shape)));
for (const slices of [[[2, 2]], [[4, 4]], [[0, 5]], [0.5], [0, 0, 0], ['...', 1, '...'], [4], [-5], [[0, 4, 0]], [[-5, 2]], [[0, -5]],
                      [[1]], [[0, 1, 1, 1]], [[null, 6, -1]], [[null, -6, -1]], ['...', [0, 7]], ['new', 0, 0, 0]])
  refused('sliceElems', {a_shape: [4, 6], slices}, () => zeros([4, 6]).sliceElems(...slices.map(undef)));
for (const axes of [[0, 0], [2], [0, -1], [1, 0, 2], [1, 1, 5]]) refused('transpose', {a_shape: [4, 6], axes}, () => zeros([4, 6]).transpose(...axes));
for (const shape of [[5, -1], [5, 5], [-2, 12], [-1, -1], [0, 24], [0, -1], [24, 1, 2]]) refused('reshape', {a_shape: [4, 6], shape}, () => zeros([4, 6]).reshape(...shape));
for (const [axis, shapes] of [[0, [[4, 6], [4, 5]]], [1, [[4, 6], [3, 6]]], [2, [[4, 6], [4, 6]]], [-3, [[4, 6], [4, 6]]], [0, [[4, 6], [6]]], [0, [[4, 6], [4, 6], [2, 4, 6]]]])
  refused('concat', {axis, shapes}, () => nd.concat(axis, shapes.map(zeros)));
for (const [axis, shapes] of [[3, [[4, 6], [4, 6]]], [-4, [[4, 6], [4, 6]]], [0, [[4, 6], [4, 5]]], [1, [[4, 6], [6]]]])
  refused('stack', {axis, shapes}, () => nd.stack(axis, shapes.map(zeros)));

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
console.log(`wrote ${count} cases, ${Object.keys(manifest.inputs).length} inputs, ${manifest.errors.length} refusals`);
for (const e of manifest.errors) console.log('refused', e.fn, JSON.stringify(e.slices || e.axes || e.shape || [e.axis, e.shapes]), '->', e.message);
