'use strict';
/* Node-side checks of schur_decomp, eigen and eigenvals (and the Francis step schur_qrfrancis) through the JS host and the N-API
 * addon. Driven by tests/test_node_schur.py.
 *   node node_schur_checks.js cpu                               (no GPU: argument checks)
 *   node node_schur_checks.js install <reference dist/nd.js>    (routing of the names, the float32 fallback)
 *   node node_schur_checks.js gpu <golden dir>                  (GPU: the three functions standalone and through install(), one
 *                                                                fixture bit for bit through the addon; never reads the reference:
 *                                                                a stand-in with its own Complex128Array stands in for nd4js)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['schur_decomp', 'eigen', 'eigenvals'];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: new Float64Array(ab), shape, complex: descr === '<c16'};
}
const sameValues = (a, b, what) => { assert.strictEqual(a.length, b.length, what); for (let i = 0; i < a.length; i++) assert(Object.is(a[i], b[i]), `${what}: entry ${i} is ${a[i]}, the reference has ${b[i]}`); };

if (mode === 'cpu') {
  for (const n of NAMES.concat(['schur_qrfrancis'])) assert.strictEqual(typeof la[n], 'function', n);
  const W = new la.NDArray(Int32Array.of(2, 3), new Float64Array(6)), S2 = new la.NDArray(Int32Array.of(2, 2), new Float64Array(4)),
        S3 = new la.NDArray(Int32Array.of(3, 3), new Float64Array(9)), B2 = new la.NDArray(Int32Array.of(1, 2, 2), new Float64Array(4)),
        V3 = new la.NDArray(Int32Array.of(3), new Float64Array(3));
  assert.throws(() => la.schur_decomp(V3), /^Error: hessenberg_decomp\(A\): A must at least be 2D\.$/);
  assert.throws(() => la.schur_decomp(W), /^Error: hessenberg_decomp\(A\): A must be square\.$/);
  assert.throws(() => la.eigen(W), /^Error: A is not square$/);
  assert.throws(() => la.eigenvals(W), /^Error: A is not square$/);
  assert.throws(() => la.schur_qrfrancis(W, W), /^Error: Q is not square\.$/);
  assert.throws(() => la.schur_qrfrancis(S2, B2), /^Error: Q\.ndim != H\.ndim\.$/);
  assert.throws(() => la.schur_qrfrancis(S2, S3), /^Error: Q\.shape != H\.shape\.$/);
  assert.throws(() => la.eigen(S2), /complex128 needs the host nd4js module/);       // the standalone module has no complex arrays
  assert.throws(() => la.eigenvals(S2), /complex128 needs the host nd4js module/);
  console.log('node schur cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {};
  for (const n of NAMES) before[n] = nd.la[n];
  const L = la.install(nd, {}).la;
  for (const n of NAMES) { assert.strictEqual(typeof L[n], 'function', n); assert.strictEqual(L.__nd4hip_original__[n], before[n], n); assert.notStrictEqual(L[n], before[n], n); }
  const F = nd.array('float32', [[1, 2], [3, 4]]);                                  // float32 is forwarded to the host module
  assert.strictEqual(L.schur_decomp(F)[1].dtype, 'float32');
  assert.strictEqual(L.eigenvals(F).shape[0], 2);
  assert.strictEqual(L.eigen(F)[1].shape[1], 2);
  // one host matrix up to the crossover N = 128 is the host module's own call: its bits
  const S = nd.array('float64', [[4, 1, 2], [1, 3, 0], [2, 0, 1]]), [Qh, Th] = before.schur_decomp(S), [Qi, Ti] = L.schur_decomp(S);
  sameValues(Qi.data, Qh.data, 'schur_decomp of one small host matrix is the host module\'s');
  sameValues(Ti.data, Th.data, 'schur_decomp of one small host matrix is the host module\'s');
  sameValues(L.eigenvals(S).data._array, before.eigenvals(S).data._array, 'eigenvals of one small host matrix is the host module\'s');
  console.log('node schur install checks ok');
} else if (mode === 'gpu') {
  class Complex128Array {
    constructor(buffer, byteOffset, length) {
      this._array = new Float64Array(buffer, byteOffset, 2 * length);
      return new Proxy(this, {get: (t, k) => typeof k !== 'symbol' && k % 1 === 0 ? [t._array[2 * k], t._array[2 * k + 1]] : t[k]});
    }
    get length() { return this._array.length / 2; }
  }
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof Complex128Array ? 'complex128' : this.data instanceof Float64Array ? 'float64' :
                         this.data instanceof Int32Array ? 'int32' : this.data instanceof Float32Array ? 'float32' : 'object'; }
  }
  const L = la.install({NDArray: HostNDArray, dt: {Complex128Array}, la: {matmul2: () => 'host'}}).la;
  const G = path.join(process.argv[3], 'schur');
  const cases = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json'))).cases;
  const arr = (name, key) => {
    const x = loadNpy(path.join(G, cases[name].files[key])), n = x.shape.reduce((a, b) => a * b, 1);
    return new HostNDArray(Int32Array.from(x.shape), x.complex ? new Complex128Array(x.data.buffer, 0, n) : x.data);
  };
  // one fixture bit for bit through the addon: the Francis step on the reference's own Hessenberg decomposition
  for (const name of ['dense_33', 'cyclic_64']) {
    const [Q, T] = L.schur_qrfrancis(arr(name, 'U'), arr(name, 'H'));
    sameValues(Q.data, arr(name, 'Q').data, name + ' Q');
    sameValues(T.data, arr(name, 'T').data, name + ' T');
  }
  { const [Q, T] = L.schur_qrfrancis(L.to_device(arr('dense_33', 'U')), L.to_device(arr('dense_33', 'H')));
    assert(T instanceof L.DeviceNDArray);
    sameValues(L.to_host(T).data, arr('dense_33', 'T').data, 'dense_33 T on device arrays');
    sameValues(L.to_host(Q).data, arr('dense_33', 'Q').data, 'dense_33 Q on device arrays'); }
  // schur_decomp, standalone and installed: the same numbers, quasi-triangular, A = Q T Q^T within four times the reference's residual
  const name = 'sym_64', c = cases[name], N = c.N, A = arr(name, 'A');
  const [Q, T] = L.schur_decomp(A), [Q1, T1] = la.schur_decomp(new la.NDArray(Int32Array.of(N, N), A.data));
  sameValues(Q.data, Q1.data, 'schur_decomp Q standalone / installed');
  sameValues(T.data, T1.data, 'schur_decomp T standalone / installed');
  for (let i = 0; i < N; i++) for (let j = 0; j + 1 < i; j++) assert(T.data[N * i + j] === 0, 'T below the subdiagonal');
  let err = 0, nrm = 0;
  const QT = new Float64Array(N * N);
  for (let i = 0; i < N; i++) for (let k = 0; k < N; k++) { const q = Q.data[N * i + k]; for (let j = 0; j < N; j++) QT[N * i + j] += q * T.data[N * k + j]; }
  for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) { let s = 0; for (let k = 0; k < N; k++) s += QT[N * i + k] * Q.data[N * j + k]; err += (s - A.data[N * i + j]) ** 2; nrm += A.data[N * i + j] ** 2; }
  assert(Math.sqrt(err / nrm) <= Math.min(4 * c.ref_residual, 1e-10), `residual ${Math.sqrt(err / nrm)}, the reference has ${c.ref_residual}`);
  // eigenvals = the eigenvalues of eigen; every pair A v = lambda v within four times the reference's own column residual
  const lam = L.eigenvals(A), [lam2, V] = L.eigen(A);
  assert(lam.data instanceof Complex128Array && V.data instanceof Complex128Array);
  assert.deepStrictEqual(Array.from(lam.shape), [N]);
  assert.deepStrictEqual(Array.from(V.shape), [N, N]);
  sameValues(lam.data._array, lam2.data._array, 'eigenvals / eigen');
  const v = V.data._array, l = lam.data._array, na = Math.sqrt(nrm);
  let worst = 0;
  for (let col = 0; col < N; col++) {
    let r2 = 0, v2 = 0;
    for (let i = 0; i < N; i++) {
      let sr = 0, si = 0;
      for (let k = 0; k < N; k++) { sr += A.data[N * i + k] * v[2 * (k * N + col)]; si += A.data[N * i + k] * v[2 * (k * N + col) + 1]; }
      const vr = v[2 * (i * N + col)], vi = v[2 * (i * N + col) + 1];
      const rr = sr - (l[2 * col] * vr - l[2 * col + 1] * vi), ri = si - (l[2 * col] * vi + l[2 * col + 1] * vr);
      r2 += rr * rr + ri * ri; v2 += vr * vr + vi * vi;
    }
    worst = Math.max(worst, Math.sqrt(r2) / (na * Math.sqrt(v2)));
  }
  assert(worst <= Math.min(4 * c.ref_eig_residual, 1e-10), `column residual ${worst}, the reference has ${c.ref_eig_residual}`);
  const ld = L.eigenvals(L.to_device(A));
  assert(ld instanceof L.DeviceNDArray);
  sameValues(L.to_host(ld).data._array, lam.data._array, 'eigenvals on a device array');
  console.log('node schur gpu checks ok');
} else throw new Error('mode');
