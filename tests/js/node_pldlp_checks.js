'use strict';
/* Node-side checks of pldlp_decomp, pldlp_solve, pldlp_l, pldlp_d and pldlp_p through the JS host and the N-API addon. Driven by
 * tests/test_node_pldlp.py.
 *   node node_pldlp_checks.js cpu <golden dir>                  (no GPU: argument checks, the host-side pldlp_l / _d / _p on fixtures)
 *   node node_pldlp_checks.js install <reference dist/nd.js>    (routing of the five names, the float32 fallback, pldlp_l / _d / _p
 *                                                                against the host module's own)
 *   node node_pldlp_checks.js gpu <golden dir>                  (GPU: the fixtures bit for bit through the addon, host and device
 *                                                                arrays; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['pldlp_decomp', 'pldlp_solve', 'pldlp_l', 'pldlp_d', 'pldlp_p'];
const SINGULAR = '_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered.';

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: descr === '<i4' ? new Int32Array(ab) : new Float64Array(ab), shape};
}
const sameValues = (a, b, what) => { assert.strictEqual(a.length, b.length, what); for (let i = 0; i < a.length; i++) assert(Object.is(a[i], b[i]) || (a[i] === 0 && b[i] === 0), `${what}: entry ${i} is ${a[i]}, the reference has ${b[i]}`); };
const f64 = (shape, data) => new la.NDArray(Int32Array.from(shape), Float64Array.from(data));
const i32 = (shape, data) => new la.NDArray(Int32Array.from(shape), Int32Array.from(data));

/* the repo's counter-based generator (nd4js_amd/rng.py) */
function fmix32(h) { h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b); h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35); h ^= h >>> 16; return h >>> 0; }
function uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0), lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  return ((hi >>> 5) * 67108864 + (lo >>> 6)) * 2.220446049250313e-16 - 1.0;
}
function fixtures(dir) {
  const G = path.join(dir, 'pldlp'), m = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json')));
  const file = (entry, key) => loadNpy(path.join(G, entry.files[key]));
  const input = name => {                       // S of a decomposition case: its file, or the seeded families
    const c = m.cases[name], N = c.N;
    if (c.input.kind === 'file') return file(c, 'S').data;
    const a = new Float64Array(N * N);
    for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) a[N * i + j] = a[N * j + i] = uniform(c.input.seed, N * i + j);
    if (c.input.kind === 'zero_diag') for (let i = 0; i < N; i++) a[N * i + i] = 0;
    if (c.input.kind === 'kkt') for (let i = c.input.m; i < N; i++) for (let j = c.input.m; j < N; j++) a[N * i + j] = 0;
    return a;
  };
  return {m, file, input};
}

function cpuChecks(L, make, makeInt) {
  const P3 = makeInt([3], [0, 1, 2]), E3 = make([3, 3], [1, 0, 0, 0, 1, 0, 0, 0, 1]);
  for (const [fn, extra] of [[L.pldlp_l, []], [L.pldlp_d, []], [L.pldlp_p, []], [L.pldlp_solve, [make([3, 1], [1, 1, 1])]]]) {
    assert.throws(() => fn(make([3], [1, 2, 3]), P3, ...extra), /^Error: pldlp_solve\(LD,P,y\): LD must be at least 2D\.$/);
    assert.throws(() => fn(make([3, 2], [1, 2, 3, 4, 5, 6]), P3, ...extra), /^Error: pldlp_solve\(LD,P,y\): LD must be square\.$/);
    assert.throws(() => fn(E3, makeInt([2], [0, 1]), ...extra), /^Error: pldlp_solve\(LD,P,y\): LD and P shape mismatch\.$/);
  }
  assert.throws(() => L.pldlp_solve(E3, P3, make([3], [1, 1, 1])), /^Error: pldlp_solve\(LD,P,y\): y must be at least 2D\.$/);
  assert.throws(() => L.pldlp_solve(E3, P3, make([2, 1], [1, 1])), /^Error: pldlp_solve\(LD,P,y\): LD and y shape mismatch\.$/);
  assert.throws(() => L.pldlp_solve(E3), /^Error: Assertion failed\.$/);
  assert.throws(() => L.pldlp_decomp(make([2, 3], [1, 2, 3, 4, 5, 6])), /^Error: Last two dimensions must be quadratic\.$/);
  // an invalid P is refused on the host, before any device work (there is no device in this mode)
  for (const [bad, msg] of [[[~0, 1, 2], /P is invalid\./], [[0, ~1, ~2], /P is invalid\./], [[0, 1, 3], /out-of-bounds indices\./],
                            [[0, ~5, 2], /P is invalid\.|out-of-bounds/], [[0, 1, 1], /duplicate indices\./]]) {
    assert.throws(() => L.pldlp_p(E3, makeInt([3], bad)), msg);
    assert.throws(() => L.pldlp_solve(E3, makeInt([3], bad), make([3, 1], [1, 1, 1])), msg);
    assert.throws(() => L.pldlp_solve([E3, makeInt([3], bad)], make([3, 1], [1, 1, 1])), msg);
  }
  // LD = [[2, 0, 0], [5, 3, 0], [7, 4, 6]] with rows (1, 2) a 2x2 block
  const LD = make([3, 3], [2, 0, 0, 5, 3, 0, 7, 4, 6]), P = makeInt([3], [2, 0, ~1]);
  assert.deepStrictEqual(Array.from(L.pldlp_l(LD, P).data), [1, 0, 0, 5, 1, 0, 7, 0, 1]);
  assert.deepStrictEqual(Array.from(L.pldlp_d(LD, P).data), [2, 0, 0, 0, 3, 4, 0, 4, 6]);
  assert.deepStrictEqual(Array.from(L.pldlp_p(LD, P).data), [2, 0, 1]);
  assert.deepStrictEqual(Array.from(L.pldlp_l([LD, P]).data), [1, 0, 0, 5, 1, 0, 7, 0, 1]);
  // broadcasting: LD [3, 3] against P [2, 3]
  const P2 = makeInt([2, 3], [2, 0, ~1, 0, 1, 2]), L2 = L.pldlp_l(LD, P2), D2 = L.pldlp_d(LD, P2);
  assert.deepStrictEqual(Array.from(L2.shape), [2, 3, 3]);
  assert.deepStrictEqual(Array.from(L2.data), [1, 0, 0, 5, 1, 0, 7, 0, 1, 1, 0, 0, 5, 1, 0, 7, 4, 1]);
  assert.deepStrictEqual(Array.from(D2.data), [2, 0, 0, 0, 3, 4, 0, 4, 6, 2, 0, 0, 0, 3, 0, 0, 0, 6]);
  assert.throws(() => L.pldlp_l(make([2, 3, 3], new Float64Array(18)), makeInt([3, 3], new Int32Array(9))), /^Error: Shapes are not broadcast-compatible\.$/);
}

if (mode === 'cpu') {
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  cpuChecks(la, f64, i32);
  assert.throws(() => la.pldlp_decomp(f64([2, 2], [1, 0, 0, 1]), {tier: 'mfma'}), /unknown tier mfma/);
  // pldlp_l / _d / _p on fixtures: L D L^T rebuilds the permuted matrix
  const {m, file, input} = fixtures(process.argv[3]);
  for (const name of ['dense_17', 'kkt_33', 'antidiag_17', 'ties_33']) {
    const c = m.cases[name], N = c.N, LD = file(c, 'LD'), P = file(c, 'P'), S = input(name);
    const Lm = la.pldlp_l(f64([N, N], LD.data), i32([N], P.data)).data, D = la.pldlp_d(f64([N, N], LD.data), i32([N], P.data)).data,
          p = la.pldlp_p(f64([N, N], LD.data), i32([N], P.data)).data;
    const LDm = new Float64Array(N * N);
    for (let i = 0; i < N; i++) for (let k = 0; k < N; k++) { const x = Lm[N * i + k]; if (x !== 0) for (let j = 0; j < N; j++) LDm[N * i + j] += x * D[N * k + j]; }
    let err = 0, nrm = 0;
    for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) {
      let s = 0; for (let k = 0; k < N; k++) s += LDm[N * i + k] * Lm[N * j + k];
      err += (s - S[N * p[i] + p[j]]) ** 2; nrm += S[N * p[i] + p[j]] ** 2;
    }
    assert(Math.sqrt(err / nrm) <= 1e-10, `${name}: L D L^T is off by ${Math.sqrt(err / nrm)}`);
  }
  console.log('node pldlp cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {};
  for (const n of NAMES) before[n] = nd.la[n];
  const L = la.install(nd, {}).la;
  for (const n of NAMES) { assert.strictEqual(typeof L[n], 'function', n); assert.strictEqual(L.__nd4hip_original__[n], before[n], n); assert.notStrictEqual(L[n], before[n], n); }
  cpuChecks(L, (shape, data) => new nd.NDArray(Int32Array.from(shape), Float64Array.from(data)), (shape, data) => new nd.NDArray(Int32Array.from(shape), Int32Array.from(data)));
  const F = nd.array('float32', [[0, 1], [1, 0]]);                                  // float32 is forwarded to the host module
  assert.strictEqual(L.pldlp_decomp(F)[0].dtype, 'float32');
  // the host-side functions give what the host module's own give, on its own factorisation with broadcasting
  const S = nd.array('float64', [[0, 2, 1, 3], [2, 0, 4, 1], [1, 4, 1, 2], [3, 1, 2, 0]]), [LD, P] = before.pldlp_decomp(S);
  const P2 = new nd.NDArray(Int32Array.of(2, 4), Int32Array.from([...P.data, ...P.data]));
  for (const n of ['pldlp_l', 'pldlp_d', 'pldlp_p']) {
    sameValues(L[n](LD, P).data, before[n](LD, P).data, n);
    sameValues(L[n]([LD, P]).data, before[n]([LD, P]).data, n + ' ([LD, P])');
    const a = L[n](LD, P2), b = before[n](LD, P2);
    assert.deepStrictEqual(Array.from(a.shape), Array.from(b.shape), n + ' broadcast shape');
    sameValues(a.data, b.data, n + ' broadcast');
  }
  console.log('node pldlp install checks ok');
} else if (mode === 'gpu') {
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof Float64Array ? 'float64' : this.data instanceof Int32Array ? 'int32' : this.data instanceof Float32Array ? 'float32' : 'object'; }
  }
  const L = la.install({NDArray: HostNDArray, la: {matmul2: () => 'host'}}).la;
  const {m, file, input} = fixtures(process.argv[3]);
  const host = (shape, data) => new HostNDArray(Int32Array.from(shape), data);
  // the fixtures bit for bit through the addon: every complete single case on the tier AUTO takes, some on each tier by name
  let n = 0;
  for (const name of Object.keys(m.cases)) {
    const c = m.cases[name];
    if (!c.files.LD) {
      if (c.error !== null) assert.throws(() => L.pldlp_decomp(host([c.N, c.N], input(name))), e => e.message === SINGULAR + ' (matrix 0)', name);
      continue;
    }
    const shape = c.lead.concat([c.N, c.N]), S = host(shape, input(name));
    if (c.error !== null) { assert.throws(() => L.pldlp_decomp(S), e => e.message === SINGULAR + ` (matrix ${c.error_member})`, name); continue; }
    const tiers = ['dense_17', 'kkt_33', 'dense_65', 'batch_2x3x17'].includes(name) ? ['auto', 'lds', 'global', 'grid'] : ['auto'];
    for (const tier of tiers) {
      const [LD, P] = L.pldlp_decomp(S, {tier});
      assert(LD instanceof HostNDArray && P.data instanceof Int32Array);
      assert.deepStrictEqual(Array.from(P.shape), c.lead.concat([c.N]));
      sameValues(LD.data, file(c, 'LD').data, `${name} LD (${tier})`);
      sameValues(P.data, file(c, 'P').data, `${name} P (${tier})`);
      n++;
    }
  }
  assert(n >= 40);
  // device arrays in, device arrays out
  { const c = m.cases.dense_130, [LD, P] = L.pldlp_decomp(L.to_device(host([130, 130], input('dense_130'))));
    assert(LD instanceof L.DeviceNDArray && P instanceof L.DeviceNDArray && P.dtype === 'int32');
    sameValues(L.to_host(LD).data, file(c, 'LD').data, 'dense_130 LD on device arrays');
    sameValues(L.to_host(P).data, file(c, 'P').data, 'dense_130 P on device arrays');
    const y = new Float64Array(130 * 2); for (let i = 0; i < y.length; i++) y[i] = uniform(m.solves.solve_dense_129_j2.y_seed, i);
    const x = L.pldlp_solve(LD, P, L.to_device(host([130, 2], y)));
    assert(x instanceof L.DeviceNDArray);
    sameValues(L.to_host(x).data, L.pldlp_solve([L.to_host(LD), L.to_host(P)], host([130, 2], y)).data, 'solve on device and host arrays'); }
  // the solves: backward error within max(N eps, 4 x the reference's own) on every solve fixture without a broadcast batch
  for (const name of Object.keys(m.solves)) {
    const sv = m.solves[name], c = m.cases[sv.decomp], N = sv.N, J = sv.J;
    if (sv.ld_lead.length || sv.y_shape.length > 2 || c.lead.length) continue;
    const y = new Float64Array(N * J); for (let i = 0; i < y.length; i++) y[i] = uniform(sv.y_seed, i);
    const x = L.pldlp_solve(host([N, N], file(c, 'LD').data), host([N], file(c, 'P').data), host([N, J], y)).data, S = input(sv.decomp);
    let r2 = 0, s2 = 0, x2 = 0, y2 = 0;
    for (let i = 0; i < N; i++) for (let j = 0; j < J; j++) { let t = -y[J * i + j]; for (let k = 0; k < N; k++) t += S[N * i + k] * x[J * k + j]; r2 += t * t; }
    for (const v of S) s2 += v * v; for (const v of x) x2 += v * v; for (const v of y) y2 += v * v;
    const be = Math.sqrt(r2) / (Math.sqrt(s2) * Math.sqrt(x2) + Math.sqrt(y2));
    assert(be <= Math.max(N * 2.220446049250313e-16, 4 * sv.ref_backward_error), `${name}: backward error ${be}, the reference has ${sv.ref_backward_error}`);
  }
  // broadcast: one LD, P against a batch of y
  { const sv = m.solves.solve_bcast_ld_17, c = m.cases.dense_17, y = new Float64Array(4 * 17 * 2); for (let i = 0; i < y.length; i++) y[i] = uniform(sv.y_seed, i);
    const LD = host([17, 17], file(c, 'LD').data), P = host([17], file(c, 'P').data), x = L.pldlp_solve(LD, P, host([4, 17, 2], y));
    assert.deepStrictEqual(Array.from(x.shape), [4, 17, 2]);
    sameValues(x.data.subarray(3 * 34), L.pldlp_solve(LD, P, host([17, 2], y.subarray(3 * 34))).data, 'broadcast LD, P'); }
  console.log('node pldlp gpu checks ok');
} else throw new Error('mode');
