#!/usr/bin/env node
/* Golden vectors of pldlp_decomp (src/la/pldlp.js:191-222) and pldlp_solve (:519-604) from the real reference bundle.
 * Decomposition cases: LD and P in full for N <= 130; above that P in full and 4096 sampled entries of the lower triangle of LD
 * (LDidx: flat indices N*i+j, LDval). A case whose call throws stores the message as `error`. Batches are factorised member
 * by member so that the members beside a singular one keep their expected output; `error_member` is the lowest singular member
 * (its LD is NaN and its P zero in the files: never compared).
 * Inputs: 'dense', 'zero_diag' and 'kkt' cases are the lower triangle of the repo's counter-based generator nd4_uniform(seed,
 * idx) (twin of nd4js_amd/rng.py) mirrored, with the diagonal resp. the trailing block [m:, m:] zeroed, and are not stored;
 * every other input is stored as S. Solve cases run the reference's pldlp_solve on the reference's LD, P of a decomposition case
 * with y = nd4_uniform(y_seed, .) and store x together with the reference's own backward error
 * ||S x - y||_F / (||S||_F ||x||_F + ||y||_F), the largest over the batch. Only numbers are written: .npy files plus manifest.json
 * (with the sha256 of every file) under tests/golden/pldlp/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_pldlp.js
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
const OUT = path.join(ROOT, 'tests', 'golden', 'pldlp');
fs.mkdirSync(OUT, {recursive: true});
const FULL_MAX_N = 130, SAMPLES = 4096;

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
function fill(seed, n) { const a = new Float64Array(n); for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i); return a; }
function symmetric(seed, N) { const g = fill(seed, N * N), a = new Float64Array(N * N); for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) a[N * i + j] = a[N * j + i] = g[N * i + j]; return a; }

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape, descr) {
  let hdr = `{'descr': '${descr}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > (1 << 20)) throw new Error(name + ': larger than 1 MiB');
  fs.writeFileSync(path.join(OUT, name + '.npy'), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', comment: 'no fixture seed has been replaced', full_max_n: FULL_MAX_N, cases: {}, solves: {}};
const arr = (shape, data) => new nd.NDArray(Int32Array.from(shape), data);
function put(m, name, key, typed, shape, descr) {
  m.sha256[key] = npy(`${name}.${key}`, typed, shape, descr);
  m.files[key] = `${name}.${key}.npy`; m.shapes[key] = shape;
}

/* ---------- families (each symmetric) ---------- */
const FAM = {
  dense: (seed, N) => symmetric(seed, N),
  zero_diag: (seed, N) => { const a = symmetric(seed, N); for (let i = 0; i < N; i++) a[N * i + i] = 0; return a; },
  kkt: (seed, N, m) => { const a = symmetric(seed, N); for (let i = m; i < N; i++) for (let j = m; j < N; j++) a[N * i + j] = 0; return a; },
  diag_dominant: (seed, N) => { const a = symmetric(seed, N); for (let i = 0; i < N; i++) a[N * i + i] = (i % 3 === 1 ? -1 : 1) * (2 * N + i); return a; },
  antidiag: (seed, N) => { const a = new Float64Array(N * N); for (let i = 0; i < N; i++) a[N * i + N - 1 - i] = 1 + i % 2; for (let i = 0; i < N; i++) a[N * i + N - 1 - i] = a[N * (N - 1 - i) + i]; return a; },
  identity: (seed, N) => { const a = new Float64Array(N * N); for (let i = 0; i < N; i++) a[N * i + i] = 1; return a; },
  ties: (seed, N) => { const a = symmetric(seed, N); for (let i = 0; i < a.length; i++) a[i] = Math.round(3 * a[i]) + 0; return a; },
  scaled_up: (seed, N) => symmetric(seed, N).map(x => x * Math.pow(2, 400)),
  scaled_down: (seed, N) => symmetric(seed, N).map(x => x * Math.pow(2, -400)),
  subnormal: (seed, N) => symmetric(seed, N).map(x => x * Math.pow(2, -1022)),        // every entry subnormal
  subnormal_deep: (seed, N) => symmetric(seed, N).map(x => x * Math.pow(2, -1040)),   // 1 / tmp overflows: NaNs arise on the way
  inf_entry: (seed, N) => { const a = symmetric(seed, N), i = N >> 1, j = N >> 2; a[N * i + j] = a[N * j + i] = Infinity; return a; },
  nan_last: (seed, N) => { const a = FAM.diag_dominant(seed, N); a[N * N - 1] = NaN; return a; },
  zero_col_first: (seed, N) => { const a = symmetric(seed, N); for (let i = 0; i < N; i++) a[i] = a[N * i] = 0; return a; },
  zero_col_mid: (seed, N) => { const a = FAM.diag_dominant(seed, N), c = N >> 1; for (let i = 0; i < N; i++) a[N * c + i] = a[N * i + c] = 0; return a; },
  nan_col: (seed, N) => { const a = symmetric(seed, N); for (let i = 0; i < N; i++) a[i] = a[N * i] = NaN; return a; },
};
const SEEDED = {dense: 1, zero_diag: 1, kkt: 1};

/* ---------- decomposition cases ---------- */
const INPUTS = {};        // name -> {N, lead, S (flat, all members), LD, P}: for the solve cases
function factorMember(N, S) {
  try { const [LD, P] = nd.la.pldlp_decomp(arr([N, N], Float64Array.from(S))); return {LD: LD.data, P: P.data}; }
  catch (e) { return {error: e.message}; }
}
// members: [{family, seed, m?}], lead: [] for one matrix
function decompCase(name, N, lead, members) {
  const batch = members.length, S = new Float64Array(batch * N * N), LD = new Float64Array(batch * N * N), P = new Int32Array(batch * N);
  const m = {family: batch === 1 ? members[0].family : 'mixed', families: members.map(x => x.family), N, lead, files: {}, shapes: {}, sha256: {},
             error: null, error_member: null, pivots_2x2: 0, moved_rows: 0};
  const t0 = process.hrtime.bigint();
  members.forEach((mem, b) => {
    const s = FAM[mem.family](mem.seed, N, mem.m);
    S.set(s, b * N * N);
    const f = factorMember(N, s);
    if (f.error) {
      if (m.error === null) { m.error = f.error; m.error_member = b; }
      LD.fill(NaN, b * N * N, (b + 1) * N * N);
    } else {
      LD.set(f.LD, b * N * N); P.set(f.P, b * N);
      for (let i = 0; i < N; i++) { if (f.P[i] < 0) m.pivots_2x2++; if ((f.P[i] < 0 ? ~f.P[i] : f.P[i]) !== i) m.moved_rows++; }
    }
  });
  m.ref_seconds = Number(process.hrtime.bigint() - t0) / 1e9;
  if (batch === 1 && SEEDED[members[0].family]) m.input = Object.assign({kind: members[0].family, seed: members[0].seed}, members[0].m !== undefined ? {m: members[0].m} : {});
  else { m.input = {kind: 'file'}; put(m, name, 'S', S, lead.concat([N, N]), '<f8'); }
  if (!(batch === 1 && m.error !== null)) {
    put(m, name, 'P', P, lead.concat([N]), '<i4');
    if (N <= FULL_MAX_N) put(m, name, 'LD', LD, lead.concat([N, N]), '<f8');
    else {
      if (batch !== 1) throw new Error(name + ': sampled batches are not supported');
      const idx = new Int32Array(SAMPLES), val = new Float64Array(SAMPLES);
      for (let q = 0; q < SAMPLES; q++) {
        let i = hashIdx(members[0].seed, 2 * q, N), j = hashIdx(members[0].seed, 2 * q + 1, N);
        if (j > i) { const t = i; i = j; j = t; }
        idx[q] = N * i + j; val[q] = LD[N * i + j];
      }
      put(m, name, 'LDidx', idx, [SAMPLES], '<i4'); put(m, name, 'LDval', val, [SAMPLES], '<f8');
    }
  }
  manifest.cases[name] = m;
  INPUTS[name] = {N, lead, S, LD, P};
  console.log('wrote', name, m.error ? 'ERROR@' + m.error_member : '', '2x2:', m.pivots_2x2, 'moved:', m.moved_rows, m.ref_seconds.toFixed(4) + ' s');
  return m;
}

let s = 12000;
const one = (name, family, N, extra) => decompCase(name, N, [], [Object.assign({family, seed: s++}, extra || {})]);
// sizes 1, 2, 3, 17, 33, both sides of 64 (the small LDS instance) and of 128 (the LDS limit), 130
for (const N of [1, 2, 3, 17, 33, 63, 64, 65, 127, 128, 129, 130]) one(`dense_${N}`, 'dense', N);
for (const N of [200, 293]) one(`dense_${N}`, 'dense', N);                 // sampled: above one update tile of the GRID tier, odd remainder
for (const N of [2, 3, 17, 33, 128]) one(`zero_diag_${N}`, 'zero_diag', N);
for (const N of [3, 17, 33, 129]) one(`kkt_${N}`, 'kkt', N, {m: N - Math.floor(N / 3)});
for (const N of [3, 17, 33, 65]) one(`diag_dominant_${N}`, 'diag_dominant', N);
for (const N of [2, 17, 33]) one(`antidiag_${N}`, 'antidiag', N);
for (const N of [1, 2, 17]) one(`identity_${N}`, 'identity', N);
for (const N of [3, 17, 33]) one(`ties_${N}`, 'ties', N);
for (const N of [17, 33]) { one(`scaled_up_${N}`, 'scaled_up', N); one(`scaled_down_${N}`, 'scaled_down', N); one(`subnormal_${N}`, 'subnormal', N); }
one('subnormal_deep_17', 'subnormal_deep', 17);
for (const N of [17, 33]) one(`inf_entry_${N}`, 'inf_entry', N);
for (const N of [1, 2, 17, 33]) {
  const m = one(`nan_last_${N}`, 'nan_last', N), I = INPUTS[`nan_last_${N}`];
  if (m.error !== null) throw new Error('nan_last must factorise');
  for (let i = 0; i < N * N - 1; i++) if (I.LD[i] !== I.LD[i]) throw new Error('nan_last: a NaN away from the last diagonal element');
  if (I.LD[N * N - 1] === I.LD[N * N - 1]) throw new Error('nan_last: the last diagonal element must be NaN');
}
for (const N of [2, 17, 33]) { if (one(`zero_col_first_${N}`, 'zero_col_first', N).error === null) throw new Error('zero column must throw'); }
for (const N of [17]) one(`zero_col_mid_${N}`, 'zero_col_mid', N);
for (const N of [2, 17, 33]) { if (one(`nan_col_${N}`, 'nan_col', N).error === null) throw new Error('NaN column must throw'); }
{ const m = decompCase('zero_1', 1, [], [{family: 'zero_col_first', seed: s++}]); if (m.error !== null) throw new Error('[[0]] must factorise'); }
// batches whose members come from different families
decompCase('batch_2x3x17', 17, [2, 3], ['dense', 'zero_diag', 'antidiag', 'ties', 'diag_dominant', 'scaled_up'].map(family => ({family, seed: s++, m: 12})));
decompCase('batch_singular_5x17', 17, [5], ['dense', 'kkt', 'zero_diag', 'zero_col_first', 'ties'].map(family => ({family, seed: s++, m: 12})));
decompCase('batch_singular_4x65', 65, [4], ['nan_col', 'dense', 'zero_col_first', 'kkt'].map(family => ({family, seed: s++, m: 44})));
decompCase('batch_3x129', 129, [3], ['dense', 'zero_diag', 'kkt'].map(family => ({family, seed: s++, m: 86})));

/* ---------- solve cases ---------- */
function fro(a) { let t = 0; for (const x of a) t += x * x; return Math.sqrt(t); }
function backwardError(N, J, S, x, y) {
  const r = new Float64Array(N * J);
  for (let i = 0; i < N; i++) for (let k = 0; k < N; k++) { const a = S[N * i + k]; for (let j = 0; j < J; j++) r[J * i + j] += a * x[J * k + j]; }
  for (let i = 0; i < N * J; i++) r[i] -= y[i];
  return fro(r) / (fro(S) * fro(x) + fro(y));
}
// ldLead / yLead: leading shapes taken from the decomposition case (its own lead, or [] = its first member) and of y
function solveCase(name, decomp, J, ldLead, yLead) {
  const I = INPUTS[decomp], N = I.N, nLD = ldLead.reduce((a, b) => a * b, 1), nY = yLead.reduce((a, b) => a * b, 1);
  const y_seed = s++, y = fill(y_seed, nY * N * J);
  const LD = arr(ldLead.concat([N, N]), I.LD.slice(0, nLD * N * N)), P = arr(ldLead.concat([N]), I.P.slice(0, nLD * N));
  const X = nd.la.pldlp_solve(LD, P, arr(yLead.concat([N, J]), y));
  const m = {decomp, N, J, ld_lead: ldLead, y_seed, y_shape: yLead.concat([N, J]), files: {}, shapes: {}, sha256: {}};
  const batch = Math.max(nLD, nY);
  let worst = 0;
  for (let b = 0; b < batch; b++) {
    const bl = nLD === 1 ? 0 : b, by = nY === 1 ? 0 : b;
    worst = Math.max(worst, backwardError(N, J, I.S.subarray(bl * N * N, (bl + 1) * N * N), X.data.subarray(b * N * J, (b + 1) * N * J), y.subarray(by * N * J, (by + 1) * N * J)));
  }
  m.ref_backward_error = worst;
  put(m, name, 'X', X.data, Array.from(X.shape), '<f8');
  manifest.solves[name] = m;
  console.log('wrote', name, 'backward error', worst.toExponential(3));
}
solveCase('solve_dd_3_j1', 'diag_dominant_3', 1, [], []);
solveCase('solve_dd_17_j2', 'diag_dominant_17', 2, [], []);
solveCase('solve_dd_33_j33', 'diag_dominant_33', 33, [], []);
solveCase('solve_dd_65_j1', 'diag_dominant_65', 1, [], []);
solveCase('solve_dense_1_j2', 'dense_1', 2, [], []);
solveCase('solve_dense_2_j1', 'dense_2', 1, [], []);
solveCase('solve_dense_33_j2', 'dense_33', 2, [], []);
solveCase('solve_dense_129_j2', 'dense_129', 2, [], []);
solveCase('solve_dense_130_j33', 'dense_130', 33, [], []);
solveCase('solve_zero_diag_17_j33', 'zero_diag_17', 33, [], []);
solveCase('solve_kkt_33_j1', 'kkt_33', 1, [], []);
solveCase('solve_kkt_129_j2', 'kkt_129', 2, [], []);
solveCase('solve_antidiag_17_j2', 'antidiag_17', 2, [], []);
solveCase('solve_identity_17_j1', 'identity_17', 1, [], []);
solveCase('solve_ties_17_j1', 'ties_17', 1, [], []);
solveCase('solve_scaled_up_17_j2', 'scaled_up_17', 2, [], []);
solveCase('solve_scaled_down_33_j2', 'scaled_down_33', 2, [], []);
solveCase('solve_bcast_ld_17', 'dense_17', 2, [], [4]);                  // one LD, P against a batch of y
solveCase('solve_bcast_y_2x3x17', 'batch_2x3x17', 1, [2, 3], []);        // a batch of LD, P against one y
solveCase('solve_batch_2x3x17_j33', 'batch_2x3x17', 33, [2, 3], [2, 3]);

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
