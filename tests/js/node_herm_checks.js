'use strict';
/* Node-side checks of eigen_herm / eigenvals_herm through the JS host and the N-API addon. Driven by tests/test_node_herm.py.
 *   node node_herm_checks.js cpu                 (no GPU: the argument errors)
 *   node node_herm_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python result)
 * complex128 lives in the host module's Complex128Array: a small host module with its own NDArray and Complex128Array (the
 * reference's layout: `_array` of interleaved doubles) stands in for nd4js, as in node_zmatmul_checks.js.
 */
const fs = require('fs'), path = require('path');
const base = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_herm', 'eigenvals_herm'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

class Complex128Array {
  constructor(buffer, byteOffset, length) { this._array = new Float64Array(buffer, byteOffset, 2 * length); }
  get length() { return this._array.length / 2; }
}
class HostNDArray {
  constructor(shape, data) { this.shape = shape; this.data = data; }
  get ndim() { return this.shape.length; }
  get dtype() { return this.data instanceof Complex128Array ? 'complex128' : this.data instanceof Float64Array ? 'float64' : this.data instanceof Int32Array ? 'int32' : 'object'; }
}
const la = base.install({NDArray: HostNDArray, dt: {Complex128Array}, la: {matmul2: () => 'host'}}).la;
const zarr = (shape, f64) => new HostNDArray(Int32Array.from(shape), new Complex128Array(f64.buffer, f64.byteOffset, f64.length / 2));
const zeye = N => { const d = new Float64Array(2 * N * N); for (let i = 0; i < N; i++) d[2 * (i * N + i)] = 1; return zarr([N, N], d); };

function argumentErrors() {
  for (const fn of NAMES) {
    assert(!Object.keys(la).includes(fn) && typeof la[fn] === 'function' && typeof base[fn] === 'function', `${fn}: a non-enumerable extension`);
    // a real matrix is sent to eigen_sym
    assert.throws(() => la[fn](new HostNDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, 0, 1))), err => err instanceof TypeError && /goes to eigen_sym/.test(err.message), fn);
    assert.throws(() => la[fn]([[1, 2], [2, 1]]), /goes to eigen_sym/, fn);
    assert.throws(() => la[fn](zarr([3], new Float64Array(6))), /H\.ndim must be at least 2/, fn);
    assert.throws(() => la[fn](zarr([2, 3], new Float64Array(12))), /H must be quadratic/, fn);
    for (const bad of [[3, 2], [0, 5], [-1, 2], [0.5, 2], [1], 3, 'ab'])
      assert.throws(() => la[fn](zeye(4), {subset: bad}), /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= N/, `${fn} ${JSON.stringify(bad)}`);
    assert.throws(() => la[fn](zeye(4), {subset: [2, 2]}), /is empty, and an NDArray has no axis of length 0/, fn);
    // the standalone module has no complex arrays: refused clearly, after the argument checks
    const z = {shape: Int32Array.of(2, 2), ndim: 2, data: {_array: new Float64Array(8)}, dtype: 'complex128'};
    assert.throws(() => base[fn](z), /complex128 needs the host nd4js module \(install\(nd\)\)/, fn);
    assert.throws(() => base[fn](z, {subset: [1, 0]}), /subset must be/, fn);
  }
}

if (mode === 'cpu') {
  argumentErrors();
  console.log('node herm cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const shape = c.shape, N = shape[shape.length - 1], k = c.subset ? c.subset[1] - c.subset[0] : N;
    const data = Float64Array.from(c.H), H = zarr(shape, data), keep = Float64Array.from(data);
    const opts = c.subset ? {subset: c.subset} : undefined;
    const lamWant = Float64Array.from(c.lam), vWant = Float64Array.from(c.V), lead = shape.slice(0, shape.length - 2);
    const [lam, V] = la.eigen_herm(H, opts);
    assert(lam instanceof HostNDArray && V instanceof HostNDArray && V.data instanceof Complex128Array && lam.data instanceof Float64Array, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(lam.shape), lead.concat([k]), name); assert.deepStrictEqual(Array.from(V.shape), lead.concat([N, k]), name);
    assert(sameBits(lam.data, lamWant) && sameBits(V.data._array, vWant), name + ': other bits than the Python result');
    assert(sameBits(data, keep), name + ': H was written');
    assert(sameBits(la.eigenvals_herm(H, opts).data, lamWant), name + ': eigenvals_herm has other bits');
    const Hd = la.to_device(H), [ld, Vd] = la.eigen_herm(Hd, opts), l2 = la.eigenvals_herm(Hd, opts);
    assert(ld instanceof base.DeviceNDArray && Vd instanceof base.DeviceNDArray && l2 instanceof base.DeviceNDArray, name + ' device in, device out');
    assert(Vd.dtype === 'complex128' && ld.dtype === 'float64', name);
    assert.deepStrictEqual(Array.from(Vd.shape), lead.concat([N, k]), name);
    assert(sameBits(la.to_host(ld).data, lamWant) && sameBits(Vd.data._array, vWant) && sameBits(la.to_host(l2).data, lamWant), name + ' device bits');
    assert(sameBits(Hd.data._array, keep), name + ': the device H was written');
    n++;
  }
  argumentErrors();
  const bad = zarr([2, 2], Float64Array.of(1, 0, 0, 0, NaN, 0, 1, 0));
  for (const fn of NAMES) {
    assert.throws(() => la[fn](bad), /eigen_herm\(H\): H contains NaN or Infinity in its lower triangle/, fn);
    assert.throws(() => la[fn](bad, {subset: [0, 1]}), /eigen_herm\(H\): H contains NaN or Infinity in its lower triangle/, fn);
  }
  console.log('node herm gpu checks ok', n);
} else throw new Error('mode');
