'use strict';
/* Node-side checks of complex matmul2 / matmul through the JS host and the N-API addon. Driven by tests/test_node_zmatmul.py.
 *   node node_zmatmul_checks.js cpu                               (no GPU: the standalone module refuses complex input clearly)
 *   node node_zmatmul_checks.js install <reference dist/nd.js>    (routing: complex pairings go to the addon, float32 and
 *                                                                  int32 x int32 are still forwarded; with a GPU, results within
 *                                                                  1e-13 of the reference's own matmul2)
 *   node node_zmatmul_checks.js gpu <golden dir>                  (GPU: results against the reference's goldens, device arrays,
 *                                                                  refusals; never reads the reference: a small host module
 *                                                                  with its own Complex128Array stands in for nd4js)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: descr === '<i4' ? new Int32Array(ab) : new Float64Array(ab), shape, complex: descr === '<c16'};
}
/* interleaved doubles: norm-wise relative error over the entries that are finite in the reference, NaN / +-Inf positions equal */
function likeReference(got, ref, what) {
  assert.strictEqual(got.length, ref.length, what);
  let dn = 0, rn = 0;
  for (let i = 0; i < ref.length; i++) {
    const g = got[i], r = ref[i];
    if (Number.isFinite(r)) { dn += (g - r) * (g - r); rn += r * r; } else assert(Object.is(g, r) || (Number.isNaN(g) && Number.isNaN(r)), `${what}: entry ${i} is ${g}, the reference has ${r}`);
    if (Number.isFinite(r)) assert(Number.isFinite(g), `${what}: entry ${i} is ${g}, the reference has ${r}`);
  }
  assert(Math.sqrt(dn) <= 1e-13 * Math.max(Math.sqrt(rn), 1e-300), `${what}: error ${Math.sqrt(dn / Math.max(rn, 1e-300))}`);
}

if (mode === 'cpu') {
  const z = {shape: Int32Array.of(2, 2), ndim: 2, data: {_array: new Float64Array(8)}, dtype: 'complex128'};   // a host-module complex array
  assert.throws(() => la.matmul2(z, z), /^Error: nd4hip\.matmul2: complex128 needs the host nd4js module \(install\(nd\)\)/);
  assert.throws(() => la.matmul2([[1, 2], [3, 4]], z), /complex128 needs the host nd4js module/);
  assert.throws(() => la.to_device(z), /^Error: nd4hip\.to_device: complex128 needs the host nd4js module/);
  assert.throws(() => la.matmul2(z, [1, 2]), /^Error: B must be at least 2D\.$/);             // the reference's errors come first
  assert.throws(() => la.matmul2(z, [[1, 2, 3]]), /^Error: The last dimension of A and the 2nd to last dimension of B do not match\.$/);
  console.log('node zmatmul cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = nd.la.matmul2, Cx = nd.dt.Complex128Array;
  const L = la.install(nd).la;
  const gen = (n, s) => Float64Array.from({length: n}, (_, i) => Math.sin(s * 7.1 + i * 1.3));
  const zarr = (shape, s) => new nd.NDArray(Int32Array.from(shape), new Cx(gen(2 * shape.reduce((a, b) => a * b, 1), s).buffer, 0, shape.reduce((a, b) => a * b, 1)));
  const A = zarr([7, 5], 1), B = zarr([5, 6], 2), R = new nd.NDArray(Int32Array.of(5, 6), gen(30, 3)), I32 = new nd.NDArray(Int32Array.of(5, 6), Int32Array.from(gen(30, 4), x => Math.round(100 * x)));
  let ran = 0, refused = 0;
  for (const [a, b] of [[A, B], [A, R], [new nd.NDArray(Int32Array.of(6, 5), gen(30, 5)), B], [A, I32]]) {
    let got;
    try { got = L.matmul2(a, b); } catch (e) {                 // routed to the addon: without a GPU it fails loudly, never computes on the host
      assert(/ND4HIP|nd4hip|HIP device/.test(e.message) || e.code === 'ND4HIP', e.message); refused++; continue;
    }
    const ref = before(a, b);
    assert.strictEqual(got.dtype, 'complex128');
    assert(got instanceof nd.NDArray && got.data instanceof Cx);
    assert.deepStrictEqual(Array.from(got.shape), Array.from(ref.shape));
    likeReference(got.data._array, ref.data._array, 'install');
    ran++;
  }
  assert.strictEqual(ran + refused, 4);
  // unchanged: float32 in any pairing and int32 x int32 are forwarded to the host module's own function
  const F = new nd.NDArray(Int32Array.of(5, 6), Float32Array.from(gen(30, 6)));
  assert.strictEqual(L.matmul2(A, F).dtype, before(A, F).dtype);
  assert.deepStrictEqual(Array.from(L.matmul2(A, F).data._array), Array.from(before(A, F).data._array));
  const I1 = new nd.NDArray(Int32Array.of(2, 2), Int32Array.of(1, 2, 3, 4));
  assert.strictEqual(L.matmul2(I1, I1).dtype, 'int32');
  assert.deepStrictEqual(Array.from(L.matmul2(I1, I1).data), Array.from(before(I1, I1).data));
  assert.strictEqual(L.__nd4hip_original__.matmul2, before);
  // the host results are built by complexOver on the host module's own Complex128Array: pin that contract on the real class
  const f = Float64Array.of(1, -2, 3.5, 4, -0, Infinity), zc = la.complexOver(Cx, f);
  assert(zc instanceof Cx && zc.length === 3 && zc._array instanceof Float64Array, 'Complex128Array over a Float64Array');
  assert(zc._array.buffer === f.buffer && zc._array.byteOffset === 0 && zc._array.length === 6, 'no copy, 2n doubles');
  f[2] = 7;
  assert.strictEqual(zc._array[2], 7);
  assert.strictEqual(zc[1].re, 7); assert.strictEqual(zc[1].im, 4);
  const sub = la.complexOver(Cx, f.subarray(2, 6));                                  // an offset view keeps its offset
  assert(sub._array.byteOffset === 16 && sub.length === 2 && sub[1].im === Infinity);
  f[5] = 5;                                                                           // (finite again: no inf * 0 below)
  const zN = new nd.NDArray(Int32Array.of(1, 3), zc);
  assert.strictEqual(zN.dtype, 'complex128');
  assert.deepStrictEqual(Array.from(before(zN, new nd.NDArray(Int32Array.of(3, 1), Float64Array.of(1, 0, 0))).data._array), [1, -2]);
  // minWork compares real flops: a complex 2x2 product (64 flops) is below 100 and forwarded, bit for bit the reference's
  const Lm = la.install(require(process.argv[3]), {minWork: 100}).la, z2 = zarr([2, 2], 9);
  assert.deepStrictEqual(Array.from(Lm.matmul2(z2, z2).data._array), Array.from(before(z2, z2).data._array));
  console.log(`node zmatmul install checks ok (${ran} on the GPU, ${refused} refused without one)`);
} else if (mode === 'gpu') {
  // a stand-in for the host module: its own NDArray and Complex128Array (the reference's layout: `_array` of interleaved doubles)
  // like the reference's ComplexArray (src/dt/complex_array.js): (buffer, byteOffset, length), `_array`, a Proxy as the instance
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
  const forwarded = [];
  const hostLa = {matmul2: (a, b) => { forwarded.push('matmul2'); return 'host'; }, matmul: () => 'host',
                  qr_decomp: () => { forwarded.push('qr_decomp'); return 'host'; }};
  const L = la.install({NDArray: HostNDArray, dt: {Complex128Array}, la: hostLa}).la;
  const G = path.join(process.argv[3], 'zmatmul');
  const cases = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json'))).cases;
  const arr = file => {
    const x = loadNpy(path.join(G, file)), n = x.shape.reduce((a, b) => a * b, 1);
    return new HostNDArray(Int32Array.from(x.shape), x.complex ? new Complex128Array(x.data.buffer, 0, n) : x.data);
  };
  let n = 0;
  for (const [name, meta] of Object.entries(cases)) {
    if (!meta.A.file || !meta.B.file) continue;                 // generated large operands: covered by test_gpu_zmatmul.py
    const A = arr(meta.A.file), B = arr(meta.B.file), ref = loadNpy(path.join(G, meta.C));
    const C = L.matmul2(A, B);
    assert(C instanceof HostNDArray && C.data instanceof Complex128Array, name);
    assert.deepStrictEqual(Array.from(C.shape), ref.shape, name);
    likeReference(C.data._array, ref.data, name);
    // residency: both on the device, and mixed
    const dA = L.to_device(A), dB = L.to_device(B);
    for (const [x, y, tag] of [[dA, dB, 'dev'], [dA, B, 'dev x host'], [A, dB, 'host x dev']]) {
      const D = L.matmul2(x, y);
      assert(D instanceof la.DeviceNDArray && D.dtype === 'complex128', name + tag);
      assert(D.data instanceof Complex128Array, name + tag);
      assert.deepStrictEqual(Array.from(D.data._array), Array.from(C.data._array), `${name} ${tag}: bit-identical to the host call`);
    }
    n++;
  }
  assert(n >= 30, n);
  // a complex device array round trip and a chain through la.matmul (planner unchanged) with mixed residency and dtypes
  const Z = new HostNDArray(Int32Array.of(4, 3), new Complex128Array(Float64Array.from({length: 24}, (_, i) => Math.cos(i)).buffer, 0, 12));
  const dZ = L.to_device(Z);
  assert.strictEqual(dZ.dtype, 'complex128');
  assert.deepStrictEqual(Array.from(L.to_host(dZ).data._array), Array.from(Z.data._array));
  const Rm = new HostNDArray(Int32Array.of(3, 5), Float64Array.from({length: 15}, (_, i) => i - 7));
  const Zt = new HostNDArray(Int32Array.of(5, 2), new Complex128Array(Float64Array.from({length: 20}, (_, i) => Math.sin(i)).buffer, 0, 10));
  const chain = L.matmul(dZ, Rm, Zt), host = L.matmul2(L.matmul2(Z, Rm), Zt);
  assert(chain instanceof la.DeviceNDArray && chain.dtype === 'complex128');
  likeReference(chain.data._array, host.data._array, 'chain');
  // every other function refuses a complex device array, before it reads the buffer
  for (const [k, args] of [['qr_decomp', [dZ]], ['lu_decomp', [dZ]], ['svd_decomp', [dZ]], ['det', [dZ]], ['norm', [dZ]],
                           ['tril_solve', [dZ, Rm]], ['cholesky_decomp', [dZ]], ['rrqr_decomp', [dZ]], ['lu_solve', [[dZ, dZ], dZ]]])
    assert.throws(() => L[k](...args), new RegExp(`^Error: nd4hip\\.${k}: complex128 device arrays are not accelerated`), k);
  // unchanged routing: float32 and int32 x int32 are forwarded to the host module; complex host input to qr_decomp as well
  const F = new HostNDArray(Int32Array.of(3, 3), new Float32Array(9)), I1 = new HostNDArray(Int32Array.of(3, 3), new Int32Array(9));
  assert.strictEqual(L.matmul2(Z, F), 'host');
  assert.strictEqual(L.matmul2(I1, I1), 'host');
  assert.strictEqual(L.qr_decomp(Z), 'host');
  assert.deepStrictEqual(forwarded, ['matmul2', 'matmul2', 'qr_decomp']);
  dZ.dispose();
  console.log(`node zmatmul gpu checks ok (${n} golden cases)`);
} else {
  throw new Error('mode: cpu | install <bundle> | gpu <golden>');
}
