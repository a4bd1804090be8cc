'use strict';
/* Node-side checks of herm_cholesky_decomp / herm_cholesky_solve / eigen_herm_gen / eigenvals_herm_gen through the JS host and the
 * N-API addon. Driven by tests/test_node_hegv.py.
 *   node node_hegv_checks.js cpu                 (no GPU: the names, the non-enumerability, the argument errors)
 *   node node_hegv_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python result)
 * complex128 lives in the host module's Complex128Array: a small host module with its own NDArray and Complex128Array (the
 * reference's layout: `_array` of interleaved doubles) stands in for nd4js, as in node_herm_checks.js.
 */
const fs = require('fs'), path = require('path');
const base = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const EIG = ['eigen_herm_gen', 'eigenvals_herm_gen'], NAMES = EIG.concat(['herm_cholesky_decomp', 'herm_cholesky_solve']);
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
const hostLa = {matmul2: () => 'host'};
const la = base.install({NDArray: HostNDArray, dt: {Complex128Array}, la: hostLa}).la;
const zarr = (shape, f64) => new HostNDArray(Int32Array.from(shape), new Complex128Array(f64.buffer, f64.byteOffset, f64.length / 2));
const rarr = (shape, f64) => new HostNDArray(Int32Array.from(shape), f64);
const zeye = N => { const d = new Float64Array(2 * N * N); for (let i = 0; i < N; i++) d[2 * (i * N + i)] = 1; return zarr([N, N], d); };

function argumentErrors() {
  // Object.keys(nd.la) stays what it was: the routed functions of the host module and nothing of this family
  assert(Object.keys(la).includes('matmul2') && !Object.keys(la).some(k => /herm|ztril/.test(k)), 'Object.keys(nd.la) stays unchanged');
  for (const fn of NAMES)
    assert(!Object.keys(la).includes(fn) && typeof la[fn] === 'function' && typeof base[fn] === 'function' && la[fn].name === fn, `${fn}: a non-enumerable extension`);
  const real = rarr([2, 2], Float64Array.of(1, 0, 0, 1));
  for (const fn of EIG) {
    assert.throws(() => la[fn](real, zeye(2)), err => err instanceof TypeError && /goes to eigen_sym_gen/.test(err.message), fn);
    assert.throws(() => la[fn](zeye(2), real), err => err instanceof TypeError && /goes to eigen_sym_gen/.test(err.message), fn);
    assert.throws(() => la[fn](zarr([3], new Float64Array(6)), zeye(3)), /A\.ndim must be at least 2/, fn);
    assert.throws(() => la[fn](zarr([2, 3], new Float64Array(12)), zeye(3)), /A must be quadratic/, fn);
    assert.throws(() => la[fn](zeye(4), zeye(3)), /B\.shape must be A\.shape or A\.shape\.slice\(-2\)/, fn);
    assert.throws(() => la[fn](zeye(4), zarr([2, 4, 4], new Float64Array(64))), /B\.shape must be A\.shape/, fn);
    for (const bad of [[3, 2], [0, 5], [-1, 2], [0.5, 2], [1], 3, 'ab'])
      assert.throws(() => la[fn](zeye(4), zeye(4), {subset: bad}), /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= N/, `${fn} ${JSON.stringify(bad)}`);
    assert.throws(() => la[fn](zeye(4), zeye(4), {subset: [2, 2]}), /is empty, and an NDArray has no axis of length 0/, fn);
    // the standalone module has no complex arrays: refused clearly, after the argument checks
    const z = {shape: Int32Array.of(2, 2), ndim: 2, data: {_array: new Float64Array(8)}, dtype: 'complex128'};
    assert.throws(() => base[fn](z, z), /complex128 needs the host nd4js module \(install\(nd\)\)/, fn);
    assert.throws(() => base[fn](z, z, {subset: [1, 0]}), /subset must be/, fn);
  }
  assert.throws(() => la.herm_cholesky_decomp(real), err => err instanceof TypeError && /goes to cholesky_decomp/.test(err.message));
  assert.throws(() => la.herm_cholesky_decomp(zarr([2, 3], new Float64Array(12))), /H must be quadratic/);
  assert.throws(() => la.herm_cholesky_decomp(zarr([3], new Float64Array(6))), /H\.ndim must be at least 2/);
  assert.throws(() => la.herm_cholesky_solve(real, zeye(2)), err => err instanceof TypeError && /goes to cholesky_solve/.test(err.message));
  assert.throws(() => la.herm_cholesky_solve(zeye(2), new HostNDArray(Int32Array.of(2, 2), Int32Array.of(1, 0, 0, 1))), /Y must be complex128 or float64/);
  assert.throws(() => la.herm_cholesky_solve(zeye(2), zeye(3)), /L and Y don't match/);
  assert.throws(() => la.herm_cholesky_solve(zeye(2), zarr([2], new Float64Array(4))), /Y\.ndim must be at least 2/);
  assert.throws(() => la.herm_cholesky_solve(zarr([3, 2, 2], new Float64Array(24)), zarr([2, 2, 2], new Float64Array(16))), /leading dimensions of Y or be \[N, N\]/);
}

if (mode === 'cpu') {
  argumentErrors();
  console.log('node hegv cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const shape = c.shape, N = shape[shape.length - 1], k = c.subset ? c.subset[1] - c.subset[0] : N;
    const dataA = Float64Array.from(c.A), dataB = Float64Array.from(c.B), A = zarr(shape, dataA), B = zarr(c.shapeB, dataB);
    const keepA = Float64Array.from(dataA), keepB = Float64Array.from(dataB);
    const opts = c.subset ? {subset: c.subset} : undefined;
    const lamWant = Float64Array.from(c.lam), xWant = Float64Array.from(c.X), lWant = Float64Array.from(c.L), sWant = Float64Array.from(c.S);
    const lead = shape.slice(0, shape.length - 2);
    const [lam, X] = la.eigen_herm_gen(A, B, opts);
    assert(lam instanceof HostNDArray && X instanceof HostNDArray && X.data instanceof Complex128Array && lam.data instanceof Float64Array, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(lam.shape), lead.concat([k]), name); assert.deepStrictEqual(Array.from(X.shape), lead.concat([N, k]), name);
    assert(sameBits(lam.data, lamWant) && sameBits(X.data._array, xWant), name + ': other bits than the Python result');
    assert(sameBits(la.eigenvals_herm_gen(A, B, opts).data, lamWant), name + ': eigenvals_herm_gen has other bits');
    const L = la.herm_cholesky_decomp(B);
    assert(L instanceof HostNDArray && L.data instanceof Complex128Array && sameBits(L.data._array, lWant), name + ': L has other bits');
    assert.deepStrictEqual(Array.from(L.shape), c.shapeB, name);
    const Y = zarr(c.shapeY, Float64Array.from(c.Y)), S = la.herm_cholesky_solve(L, Y);
    assert(S.data instanceof Complex128Array && sameBits(S.data._array, sWant), name + ': the solve has other bits');
    assert.deepStrictEqual(Array.from(S.shape), c.shapeY, name);
    assert(sameBits(dataA, keepA) && sameBits(dataB, keepB), name + ': an input was written');
    const Ad = la.to_device(A), Bd = la.to_device(B), [ld, Xd] = la.eigen_herm_gen(Ad, Bd, opts), l2 = la.eigenvals_herm_gen(Ad, Bd, opts);
    assert(ld instanceof base.DeviceNDArray && Xd instanceof base.DeviceNDArray && l2 instanceof base.DeviceNDArray, name + ' device in, device out');
    assert(Xd.dtype === 'complex128' && ld.dtype === 'float64', name);
    assert.deepStrictEqual(Array.from(Xd.shape), lead.concat([N, k]), name);
    assert(sameBits(la.to_host(ld).data, lamWant) && sameBits(Xd.data._array, xWant) && sameBits(la.to_host(l2).data, lamWant), name + ' device bits');
    const Ld = la.herm_cholesky_decomp(Bd), Sd = la.herm_cholesky_solve(Ld, la.to_device(Y));
    assert(Ld instanceof base.DeviceNDArray && Ld.dtype === 'complex128' && sameBits(Ld.data._array, lWant), name + ': the device L');
    assert(Sd instanceof base.DeviceNDArray && sameBits(Sd.data._array, sWant), name + ': the device solve');
    assert(sameBits(Ad.data._array, keepA) && sameBits(Bd.data._array, keepB), name + ': a device input was written');
    if (c.Sreal) {                                // a float64 Y is promoted
      const Yr = rarr(c.shapeY, Float64Array.from(c.Yreal)), want = Float64Array.from(c.Sreal);
      assert(sameBits(la.herm_cholesky_solve(L, Yr).data._array, want) && sameBits(la.herm_cholesky_solve(Ld, la.to_device(Yr)).data._array, want), name + ': real Y');
    }
    n++;
  }
  argumentErrors();
  const bad = zarr([2, 2], Float64Array.of(1, 0, 0, 0, 3, 0, 1, 0));      // [[1, .], [3, 1]]: not positive definite
  for (const fn of EIG) {
    assert.throws(() => la[fn](zeye(2), bad), /eigen_herm_gen\(A,B\): B is not positive definite\. \(matrix 0\)/, fn);
    assert.throws(() => la[fn](zarr([2, 2], Float64Array.of(1, 0, 0, 0, NaN, 0, 1, 0)), zeye(2)), /eigen_herm_gen\(A,B\): L\^-1 A L\^-H is not finite/, fn);
  }
  assert.throws(() => la.herm_cholesky_decomp(bad), /herm_cholesky_decomp\(H\): H is not positive definite\. \(matrix 0\)/);
  console.log('node hegv gpu checks ok', n);
} else throw new Error('mode');
